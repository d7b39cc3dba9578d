// sdfk_moments.inc — mass properties of a program on a grid: the integer moments M = (N, U0, U1, U2, U00, U01, U02, U11,
// U12, U22) of the inside sub-sample points of sdfk_eval_grid_occupancy's lattice, the sums of 1, u_a and u_a u_b with
// u_a = 2 (i_a k_a + j_a) + 1 (included at the end of sdfk.hip, after sdfk_occupancy.inc, whose request, tables, scratch
// tail, far rule, count kernel and slab driver — occ_request, occ_open, occ_tail, occ_slabs — it uses unchanged; the
// sample pass itself: sdfk_momdev.h; the definition for users: aegolius_amd/moments.py). No per-cell output exists. Of
// the three passes occ_slabs runs per slab, MomSums supplies what differs from occupancy:
//
//   1. centre values : occ_slabs'.
//   2. far           : after occ_slabs' count and scan, sdfk_mom_far_kernel decides again (sdfk_occ_near, the same function
//      of the same inputs: near_cells is the number occupancy reports), writes the near cells' indices to the list and adds up,
//      over the far cells on the inside, the sums of 1, i_a and i_a i_b of their CELL indices. The block sums of 1, u_a
//      and u_a u_b over the k^d samples of a cell are polynomials of degree two in (i0, i1, i2), so the host expands the
//      ten index sums into the far cells' share of M in 128-bit integers (mom_expand_far): no field evaluation, and the
//      device multiplies indices, not lattice coordinates.
//   3. sample        : sdfk_mom_sample over the list — the interpreter kernel below or the specialised flavour
//      (SDFK_FL_MOMENTS), same text, same integers.
// Both reductions keep per-lane 64-bit sums, fold them once per wave and store one partial of ten uint64 per wave with
// plain vector stores; the host adds the partials in 128 bits. mom_waves picks the number of waves so that no partial can
// wrap, and the call fails where none does. Scratch: the two partial arrays, then the lattice's tail (occ_tail).
#include "sdfk_momdev.h"

template <int NC, int NV, typename SRC>
__global__ __launch_bounds__(SDFK_OCC_BLOCK) void sdfk_mom_interp_kernel(const uint2* __restrict__ code, int n_instr,
                                                                        const float* __restrict__ prm,
                                                                        const float* __restrict__ tab, int result_reg, SRC src,
                                                                        sdfk_occgrid grid, unsigned waves,
                                                                        unsigned long long* __restrict__ partial) {
    const SdfkInterpField<NC, NV> field = {code, n_instr, prm, tab, result_reg};
    sdfk_mom_sample(src, field, grid, waves, partial);
}

// blk: the exclusive offsets of the runs' near cells. A wave owns the runs wave, wave + waves, ...; near cells go to the
// list (ascending), far cells on the inside add 1, i_a, i_a i_b to the lane's sums; partial: SDFK_MOM_SUMS uint64 per wave.
__global__ __launch_bounds__(SDFK_OCC_BLOCK) void sdfk_mom_far_kernel(const float* __restrict__ centre, sdfk_occclass C,
                                                                     unsigned* __restrict__ list,
                                                                     const unsigned long long* __restrict__ blk, long long runs,
                                                                     unsigned waves, unsigned long long* __restrict__ partial) {
    const unsigned lane = sdfk_tx() & 63u;
    const long long wave = (long long)sdfk_bx() * (SDFK_OCC_BLOCK / 64) + (sdfk_tx() >> 6);
    unsigned long long m[SDFK_MOM_SUMS];
#pragma unroll
    for (int t = 0; t < SDFK_MOM_SUMS; ++t) m[t] = 0ull;
    for (long long run = wave; run < runs; run += waves) {      // (wave-uniform trip count)
        const long long begin = run * SDFK_OCC_RUN;
        SdfkOccWalk walk;
        walk.start((unsigned long long)(C.first + begin), C.n1, C.n2);
        unsigned long long at = blk[run];
        for (int r = 0; r < SDFK_OCC_RUN / 64; ++r) {
            const long long i = begin + r * 64 + lane;
            const bool active = i < C.count;
            bool near_cell = false, inside = false;
            unsigned long long i0 = 0ull;
            unsigned i1 = 0u, i2 = 0u;
            if (active) {
                walk.lane(lane, C.n1, C.n2, i0, i1, i2);
                near_cell = sdfk_occ_near(C, centre[i], i0, i1, i2, &inside);
            }
            const unsigned long long nb = __ballot(near_cell);
            const unsigned long long slot = at + (unsigned)__popcll(nb & ((1ull << lane) - 1ull));
            if (near_cell && slot < (unsigned long long)C.count) list[slot] = (unsigned)i;
            const bool add = active && !near_cell && inside;
            const unsigned v0 = add ? (unsigned)i0 : 0u, v1 = add ? i1 : 0u, v2 = add ? i2 : 0u;   // (n k < 2^31: the host's check)
            m[0] += add ? 1ull : 0ull;
            m[1] += v0;
            m[2] += v1;
            m[3] += v2;
            m[4] += (unsigned long long)v0 * v0;
            m[5] += (unsigned long long)v0 * v1;
            m[6] += (unsigned long long)v0 * v2;
            m[7] += (unsigned long long)v1 * v1;
            m[8] += (unsigned long long)v1 * v2;
            m[9] += (unsigned long long)v2 * v2;
            at += (unsigned)__popcll(nb);
            walk.advance(C.n1, C.n2);
        }
    }
#pragma unroll
    for (int t = 0; t < SDFK_MOM_SUMS; ++t) {
        const unsigned long long total = sdfk_mom_fold(m[t]);
        if (lane == 0u) partial[wave * SDFK_MOM_SUMS + t] = total;
    }
}

// ---- host side ----------------------------------------------------------------------------------
typedef unsigned __int128 mom_u128;
#define SDFK_MOM_WAVES 8192            // waves of a reduction: what the device holds at 8 waves per SIMD ...
#define SDFK_MOM_WAVES_MAX 65536       // ... and how far mom_waves may go to keep the partials from wrapping

// Waves of a reduction over `units` (groups, runs), each of which adds at most `weight` to a 64-bit sum: the smallest of
// 8192, 16384, ..., cap with ceil(units / waves) * weight < 2^63, cut to `units`; 0 if there is none.
static unsigned mom_waves(unsigned long long units, mom_u128 weight, unsigned cap) {
    for (unsigned long long waves = SDFK_MOM_WAVES;; waves *= 2) {
        const unsigned long long w = std::min<unsigned long long>(std::min<unsigned long long>(waves, cap), std::max<unsigned long long>(units, 1));
        const unsigned long long per_wave = (units + w - 1) / w;
        if ((mom_u128)per_wave * weight < ((mom_u128)1 << 63)) return (unsigned)w;
        if (w < waves) return 0u;                               // (cut by the cap or the units: more waves do not help)
    }
}
static unsigned mom_blocks(unsigned waves) { return (waves + SDFK_OCC_BLOCK / 64 - 1) / (SDFK_OCC_BLOCK / 64); }
// partials a slab of `units` can need: whole blocks
static size_t mom_partial_bytes(int64_t units) {
    const unsigned waves = (unsigned)std::min<int64_t>(std::max<int64_t>(units, 1), SDFK_MOM_WAVES_MAX);
    return occ_align((size_t)mom_blocks(waves) * (SDFK_OCC_BLOCK / 64) * SDFK_MOM_SUMS * 8);
}

// scratch layout: the sample pass's partials | the far pass's partials | the lattice's tail
extern "C" size_t sdfk_eval_grid_moments_scratch(int64_t n0, int64_t n1, int64_t n2, int64_t slab_cells) {
    if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
    const int64_t slab = occ_slab_cells(n0, n1, n2, slab_cells);
    return mom_partial_bytes(slab) + mom_partial_bytes(occ_runs(slab)) + occ_tail_bytes(slab);
}

// sum[t] += the partials of `waves` waves (device -> host; synchronises the stream)
static int mom_add_partials(const unsigned long long* d_partial, unsigned waves, hipStream_t stream, std::vector<unsigned long long>* host,
                            mom_u128* sum) {
    host->resize((size_t)waves * SDFK_MOM_SUMS);
    HIPCHK(hipMemcpyAsync(host->data(), d_partial, host->size() * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (size_t w = 0; w < waves; ++w)
        for (int t = 0; t < SDFK_MOM_SUMS; ++t) sum[t] += (*host)[w * SDFK_MOM_SUMS + t];
    return 0;
}

// The share of M of cells whose samples are all inside, from the sums I = (c, I0, I1, I2, I00, I01, I02, I11, I12, I22) of
// 1, i_a, i_a i_b over those cells. Per axis, over the k samples of cell i (u = 2 (i k + j) + 1):
//     sum 1 = k,   sum u = k^2 (2 i + 1),   sum u^2 = 4 k^3 (i^2 + i) + k (4 k^2 - 1) / 3,
// and a product of terms of different axes sums to the product of the axes' sums.
static void mom_expand_far(const mom_u128* I, const unsigned* k, mom_u128* M) {
    static const int diag[3] = {4, 7, 9}, off[3][3] = {{4, 5, 6}, {5, 7, 8}, {6, 8, 9}};
    const mom_u128 K = (mom_u128)k[0] * k[1] * k[2];
    M[0] += K * I[0];
    for (int a = 0; a < 3; ++a) {
        const mom_u128 ka = k[a], others = K / ka;
        M[1 + a] += others * ka * ka * (2 * I[1 + a] + I[0]);
        M[diag[a]] += others * (4 * ka * ka * ka * (I[diag[a]] + I[1 + a]) + ka * (4 * ka * ka - 1) / 3 * I[0]);
        for (int b = a + 1; b < 3; ++b) {
            const mom_u128 kb = k[b];
            M[off[a][b]] += K / (ka * kb) * ka * ka * kb * kb * (4 * I[off[a][b]] + 2 * I[1 + a] + 2 * I[1 + b] + I[0]);
        }
    }
}

// occ_slabs' consumer: the far cells' index sums from the second classify pass, the near cells' share of M from the sample
// pass. Each reduction is sized so that no partial can wrap (the weights and caps: sdfk_eval_grid_moments) and folded on
// the host, which is also the stream synchronisation occ_slabs asks for.
struct MomSums {
    const std::string& w;
    mom_u128 group_weight, run_weight;
    unsigned cap_groups, cap_runs;
    unsigned long long* d_part_near;
    unsigned long long* d_part_far;
    mom_u128 far_sum[SDFK_MOM_SUMS] = {}, M[SDFK_MOM_SUMS] = {};
    std::vector<unsigned long long> host;
    unsigned far_waves = 0, waves = 0;
    template <int NC, int NV, typename SRC>
    static auto interp_kernel() { return sdfk_mom_interp_kernel<NC, NV, SRC>; }
    int classify(const OccTables& t, const OccTail& s, int64_t, long long runs, unsigned) {
        far_waves = mom_waves((unsigned long long)runs, run_weight, cap_runs);
        if (!far_waves) return fail(-2, w + ": a 64-bit partial sum could wrap");
        far_waves = mom_blocks(far_waves) * (SDFK_OCC_BLOCK / 64);
        hipLaunchKernelGGL(sdfk_mom_far_kernel, dim3(far_waves / (SDFK_OCC_BLOCK / 64)), dim3(SDFK_OCC_BLOCK), 0, t.x.stream,
                           (const float*)s.d_centre, t.C, s.d_list, (const unsigned long long*)s.d_blk, runs, far_waves, d_part_far);
        return 0;
    }
    int classified(hipStream_t stream) { return mom_add_partials(d_part_far, far_waves, stream, &host, far_sum); }
    template <typename SRC>
    int sample(const OccRequest& q, const OccTables& t, SRC src, int64_t) {
        const unsigned long long groups = (src.n + q.per_wave - 1) / q.per_wave;
        waves = mom_waves(groups, group_weight, cap_groups);
        if (!waves) return fail(-2, w + ": a 64-bit partial sum could wrap");
        const unsigned blocks = mom_blocks(waves);
        waves = blocks * (SDFK_OCC_BLOCK / 64);
        return occ_sample_launch<MomSums>(q, t, src, blocks, waves, d_part_near);
    }
    int sampled(hipStream_t stream) { return mom_add_partials(d_part_near, waves, stream, &host, M); }
};

extern "C" int sdfk_eval_grid_moments(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                      const float* ax2, int64_t n2, const float* sub0, const float* sub1, const float* sub2,
                                      const float* hw0, const float* hw1, const float* hw2, int samples, float level,
                                      float lipschitz, void* d_scratch, size_t scratch_bytes, int64_t slab_cells,
                                      uint64_t* moments_out, int64_t* near_cells, float* pass_ms, void* stream_, int mode) {
    const std::string w = "sdfk_eval_grid_moments";
    OccRequest q = {p, {ax0, ax1, ax2}, {sub0, sub1, sub2}, {hw0, hw1, hw2}, {n0, n1, n2}, samples, level, lipschitz, slab_cells, mode};
    int rc = occ_request(w, 0x7fffffff, &q);
    if (rc) return rc;
    if (!d_scratch) return fail(-1, w + ": null scratch pointer");
    if (!moments_out || !near_cells) return fail(-1, w + ": null result pointer");
    if (scratch_bytes < sdfk_eval_grid_moments_scratch(n0, n1, n2, slab_cells)) return fail(-1, w + ": the scratch buffer is too small");
    // the longest axis in sub-samples: u = 2 (i k + j) + 1 < 2 n k is computed in 32 bits on the device
    const int64_t longest = std::max(std::max(n0 * q.k[0], n1 * q.k[1]), n2 * q.k[2]);
    if (longest >= (1LL << 31)) return fail(-1, w + ": an axis of 2^31 sub-samples or more");
    const int64_t slab = q.slab;
    const mom_u128 u_max = 2 * (mom_u128)longest;
    const mom_u128 group_weight = (mom_u128)std::max(q.K, 64u) * u_max * u_max;
    const mom_u128 run_weight = (mom_u128)SDFK_OCC_RUN * (mom_u128)longest * (mom_u128)longest;
    const unsigned long long slab_groups = ((unsigned long long)slab + q.per_wave - 1) / q.per_wave;
    // (groups and runs of a slab never exceed these; the partial arrays are laid out for them)
    const unsigned cap_groups = (unsigned)std::min<int64_t>(slab, SDFK_MOM_WAVES_MAX);
    const unsigned cap_runs = (unsigned)std::min<int64_t>(occ_runs(slab), SDFK_MOM_WAVES_MAX);
    if (!mom_waves(slab_groups, group_weight, cap_groups) || (q.skip && !mom_waves((unsigned long long)occ_runs(slab), run_weight, cap_runs)))
        return fail(-2, w + ": a 64-bit partial sum could wrap on a grid this long (take smaller slabs)");

    OccTables t;
    rc = occ_open(q, stream_, SDFK_FL_MOMENTS, "moments kernel", &t);
    if (rc) return rc;
    char* scratch = (char*)d_scratch;
    const size_t near_bytes = mom_partial_bytes(slab), far_bytes = mom_partial_bytes(occ_runs(slab));
    MomSums sums = {w, group_weight, run_weight, cap_groups, cap_runs, (unsigned long long*)scratch,
                    (unsigned long long*)(scratch + near_bytes)};
    rc = occ_slabs(w, q, t, occ_tail(scratch + near_bytes + far_bytes, slab), pass_ms, sums, near_cells);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(t.x.stream));                   // the tables are freed on return
    mom_expand_far(sums.far_sum, q.k, sums.M);
    for (int i = 0; i < SDFK_MOM_SUMS; ++i) {
        moments_out[2 * i] = (uint64_t)sums.M[i];
        moments_out[2 * i + 1] = (uint64_t)(sums.M[i] >> 64);
    }
    return 0;
}
