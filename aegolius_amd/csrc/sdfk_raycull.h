// sdfk_raycull.h — culling along rays: SdfkCullField, the field object of the specialised chain-mode march kernels
// (embedded text only: it needs the generated chain tables, so it follows them in the hiprtc unit — sdfk_codegen.cpp).
//
// Sphere tracing of a chain-mode program with per-wave survivor lists (emitted after the plain kernels from
// SDFK_RAYS_CULL_MIN_LEAVES members on). The wave is the brick: sdfk_march's hook hands over the points the wave is about
// to evaluate and which lanes count; the field bounds them by a sphere (c, R), evaluates every member at c — a member per
// lane, 64 per batch — and keeps member k unless e_k - m >= thr0 + 1e-6 |e_k| (the rule and the margins of
// sdfk_chain_fold_cells, word for word). The survivors go, in index order, into a list in LDS, and every lane folds the
// chain over that list: the members it leaves out are larger than the minimum at every point within R of c, so a hard
// min / max returns the same bits. sdfk_chain_tail runs per lane as in the plain body.
//   * A list is valid for points within R of c, and is kept while every active lane stays inside (1.0001 |p - c| + reach
//     <= R). R = the rounded-up radius of the points + the reach + SDFK_RAYS_LOOK * radius: a look-ahead would buy
//     evaluations without a rebuild at the price of longer lists; it is 0 (rays in the open leave any sphere worth
//     listing in one step, rays that creep stay inside the exact one), so a list is rebuilt when a lane has left it.
//   * More than SDFK_RAYS_CAP survivors: the lanes are split at the middle of their t range into two groups with a list
//     each, at most SDFK_RAYS_DEPTH deep (8 groups); a group is evaluated with the other lanes masked. What still
//     overflows — or has no finite bounds — runs every member, as the plain kernel does; so does the whole wave when its
//     groups together would cost more than that (incoherent rays of a cast), and then the next SDFK_RAYS_HOLD
//     evaluations run every member without building anything: such a wave pays for the 15 builds of a full split once
//     in five evaluations and is otherwise the plain kernel.
//   * Everything that ballots, reduces or writes a list runs in wave-uniform control flow, with every lane of the wave;
//     lanes outside `active` are kept out of the bounds by value, not by a branch.
// -DSDFK_DEBUG_RAYSTATS=1 (test aid): counts per wave into STATS, lane 0, ordinary vector atomics — see sdfk.h.
#ifndef SDFK_RAYCULL_H
#define SDFK_RAYCULL_H
#ifndef SDFK_RAYS_CAP
#define SDFK_RAYS_CAP 192        // records of one list
#endif
#ifndef SDFK_RAYS_POOL
#define SDFK_RAYS_POOL 1024      // records of all the lists of a wave
#endif
#ifndef SDFK_RAYS_LOOK
#define SDFK_RAYS_LOOK 0.0f      // look-ahead, in radii of the points' sphere (it does not pay)
#endif
#define SDFK_RAYS_GROUPS 8
#define SDFK_RAYS_HOLD 4u        // evaluations without a list after one whose lists did not pay
#define SDFK_RAYS_DEPTH 3
#define SDFK_RAYS_PLAIN 0xffffffffu
static_assert(SDFK_RAYS_GROUPS == (1 << SDFK_RAYS_DEPTH), "a binary split");
#if defined(SDFK_DEBUG_RAYSTATS) && SDFK_DEBUG_RAYSTATS
#define SDFK_RSTAT(i, v) do { if (lane == 0 && STATS) atomicAdd(STATS + (i), (unsigned long long)(v)); } while (0)
#else
#define SDFK_RSTAT(i, v) do { } while (0)
#endif
struct sdfk_raylists {           // LDS of one wave
    unsigned rec[SDFK_RAYS_POOL];
    unsigned glo[SDFK_RAYS_GROUPS], ghi[SDFK_RAYS_GROUPS];     // the lanes of group g
    unsigned goff[SDFK_RAYS_GROUPS], gcnt[SDFK_RAYS_GROUPS];   // its list (gcnt = SDFK_RAYS_PLAIN: every member)
    unsigned gdep[SDFK_RAYS_GROUPS];
};
static __device__ __forceinline__ void sdfk_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
static __device__ __forceinline__ unsigned sdfk_uni(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }

struct SdfkCullField {
    const float* __restrict__ PRM;
    const float* __restrict__ TAB;
    sdfk_raylists* L;
    unsigned long long* STATS;
    int lane;
    mutable V3 gc;               // the sphere of this lane's list (gR < 0: none)
    mutable float gR;
    mutable unsigned ng;         // groups (wave-uniform)
    mutable unsigned hold;       // evaluations still to run without a list (wave-uniform)

    // one list: the lanes of `cur`, records at L->rec[base ...] (at most cap). -> survivors, or SDFK_RAYS_PLAIN (no finite bounds)
    __device__ __forceinline__ unsigned build(unsigned long long cur, V3 p, float reach, unsigned base, unsigned cap, V3& c,
                                              float& R) const {
        const bool in = (cur >> lane) & 1ull;
        const float big = 3.0e38f;
        const float xlo = -sdfk_wave_max(in ? -p.x : -big), xhi = sdfk_wave_max(in ? p.x : -big);
        const float ylo = -sdfk_wave_max(in ? -p.y : -big), yhi = sdfk_wave_max(in ? p.y : -big);
        const float zlo = -sdfk_wave_max(in ? -p.z : -big), zhi = sdfk_wave_max(in ? p.z : -big);
        c = {0.5f * xlo + 0.5f * xhi, 0.5f * ylo + 0.5f * yhi, 0.5f * zlo + 0.5f * zhi};
        const float dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
        const float r2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const bool bad = in && !(r2 < big);
        const float rad = 1.0001f * sqrtf(sdfk_wave_max(in ? r2 : 0.0f)) + 1e-30f;
        const float rch = sdfk_wave_max(in ? reach : 0.0f);
        SDFK_RSTAT(0, 1);
        if (__any(bad) || !(rad + rch < big) || !(fabsf(c.x) + fabsf(c.y) + fabsf(c.z) < big)) return SDFK_RAYS_PLAIN;
        const V3T<float> ctr = {c.x, c.y, c.z};
        // The members' values at c are needed twice, for m and for the comparison. The part of the pool that this list
        // cannot use keeps them between the two passes (a lane reads back what it wrote); members beyond it are evaluated again.
        const unsigned ncache = SDFK_RAYS_POOL - base - cap;
        float m = 3.0e38f;
        _Pragma("unroll 1") for (unsigned j0 = 0u; j0 < SDFK_NLEAF; j0 += 64u) {
            const unsigned j = j0 + (unsigned)lane;
            const bool mem = j < SDFK_NLEAF;
            float e = 3.0e38f;
            if (mem) e = SDFK_CHAIN_SGN * sdfk_leaf_rec<float>(sdfk_member_record(j), ctr, PRM, TAB);
            if (mem && j < ncache) L->rec[base + cap + j] = __builtin_bit_cast(unsigned, e);
            m = fminf(m, e);
        }
        _Pragma("unroll") for (int o = 1; o < 64; o <<= 1) m = fminf(m, __shfl_xor(m, o));
        // (no look-ahead for the stencil's list, rch > 0: the normal is its only user)
        const float rho = rad + rch + (rch > 0.0f ? 0.0f : SDFK_RAYS_LOOK * rad);
        if (!(rho < big)) return SDFK_RAYS_PLAIN;
        R = rho;
        const float cmag = 1e-6f * (fabsf(c.x) + fabsf(c.y) + fabsf(c.z) + rho);
        const float thr0 = 1.0001f * SDFK_CHAIN_KMAX * rho + SDFK_CHAIN_KMAX * cmag + 1e-6f * (1.0f + fabsf(m));
        unsigned n_out = 0u;
        _Pragma("unroll 1") for (unsigned j0 = 0u; j0 < SDFK_NLEAF; j0 += 64u) {
            const unsigned j = j0 + (unsigned)lane;
            const bool mem = j < SDFK_NLEAF;
            const unsigned rec = mem ? sdfk_member_record(j) : 0u;
            float e = 3.0e38f;
            if (mem) {
                if (j < ncache) e = __builtin_bit_cast(float, L->rec[base + cap + j]);
                else e = SDFK_CHAIN_SGN * sdfk_leaf_rec<float>(rec, ctr, PRM, TAB);
            }
            const bool run = mem && !(e - m >= thr0 + 1e-6f * fabsf(e));          // (negated: NaN keeps the member)
            const unsigned long long bits = __ballot(run);
            const unsigned pos = n_out + (unsigned)__builtin_popcountll(bits & ((1ull << lane) - 1ull));
            if (run && pos < cap) L->rec[base + pos] = rec;
            n_out += (unsigned)__builtin_popcountll(bits);
        }
        SDFK_RSTAT(1, SDFK_NLEAF + (SDFK_NLEAF > ncache ? SDFK_NLEAF - ncache : 0u));
        return n_out;
    }

    __device__ __forceinline__ void prepare(V3 p, float key, bool active, float reach) const {
        {
            const float dx = p.x - gc.x, dy = p.y - gc.y, dz = p.z - gc.z;
            const float dist = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
            const bool need = active && !(1.0001f * dist + reach <= gR);
            if (!__any(need)) return;                            // every active lane is inside the sphere of its list
        }
        gR = -1.0f;
        const unsigned long long all = __ballot(active);
        if (hold != 0u) {                                        // (wave-uniform) lists did not pay a moment ago: every member, no build
            sdfk_lds_order();
            L->glo[0] = (unsigned)all; L->ghi[0] = (unsigned)(all >> 32);
            L->goff[0] = 0u; L->gcnt[0] = SDFK_RAYS_PLAIN;
            hold = sdfk_uni(hold - 1u);
            ng = 1u;
            sdfk_lds_order();
            return;
        }
        unsigned long long cur = all;
        unsigned nq = 1u, qi = 0u, used = 0u, depth = 0u, cost = 0u;
        _Pragma("unroll 1") while (qi < nq) {
            const bool in = (cur >> lane) & 1ull;
            const unsigned cap = SDFK_RAYS_POOL - used < SDFK_RAYS_CAP ? SDFK_RAYS_POOL - used : SDFK_RAYS_CAP;
            V3 c = {0.0f, 0.0f, 0.0f};
            float R = -1.0f;
            unsigned n_out = build(cur, p, reach, used, cap, c, R);
            if (n_out != SDFK_RAYS_PLAIN && (n_out > cap || n_out == 0u)) {
                if (n_out > cap && depth < SDFK_RAYS_DEPTH && nq < SDFK_RAYS_GROUPS) {
                    const float klo = -sdfk_wave_max(in ? -key : -3.0e38f), khi = sdfk_wave_max(in ? key : -3.0e38f);
                    const float mid = 0.5f * klo + 0.5f * khi;
                    const unsigned long long lo = __ballot(in && key <= mid), hi = cur & ~lo;
                    if (lo != 0ull && hi != 0ull) {
                        ++depth;
                        L->glo[nq] = (unsigned)hi; L->ghi[nq] = (unsigned)(hi >> 32); L->gdep[nq] = depth;
                        ++nq;
                        cur = lo;
                        SDFK_RSTAT(4, 1);
                        continue;
                    }
                }
                n_out = SDFK_RAYS_PLAIN;
            }
            L->glo[qi] = (unsigned)cur; L->ghi[qi] = (unsigned)(cur >> 32);
            L->goff[qi] = used; L->gcnt[qi] = n_out;
            if (in && n_out != SDFK_RAYS_PLAIN) { gc = c; gR = R; }
            if (n_out != SDFK_RAYS_PLAIN) used += n_out;
            cost += n_out != SDFK_RAYS_PLAIN ? n_out : SDFK_NLEAF;
            ++qi;
            if (qi < nq) {
                sdfk_lds_order();
                cur = (unsigned long long)sdfk_uni(L->glo[qi]) | ((unsigned long long)sdfk_uni(L->ghi[qi]) << 32);
                depth = sdfk_uni(L->gdep[qi]);
            }
        }
        if (nq > 1u && cost >= SDFK_NLEAF) {
            // the groups together cost more than every member once (each group without a list runs them all): one group
            sdfk_lds_order();
            L->glo[0] = (unsigned)all; L->ghi[0] = (unsigned)(all >> 32);
            L->goff[0] = 0u; L->gcnt[0] = SDFK_RAYS_PLAIN;
            gR = -1.0f;
            nq = 1u;
            hold = SDFK_RAYS_HOLD;
        }
        ng = sdfk_uni(nq);
        sdfk_lds_order();
    }

    __device__ __forceinline__ float operator()(V3 p) const {
        const V3T<float> C_0 = {p.x, p.y, p.z};
        float acc = 0.0f;
        SDFK_RSTAT(5, 1);
        _Pragma("unroll 1") for (unsigned g = 0u; g < ng; ++g) {
            const unsigned long long mask = (unsigned long long)sdfk_uni(L->glo[g]) | ((unsigned long long)sdfk_uni(L->ghi[g]) << 32);
            const unsigned off = sdfk_uni(L->goff[g]), cnt = sdfk_uni(L->gcnt[g]);
            if (cnt == SDFK_RAYS_PLAIN) SDFK_RSTAT(3, 64);
            else SDFK_RSTAT(2, 64u * cnt);
            if ((mask >> lane) & 1ull) {
                float a;
                if (cnt == SDFK_RAYS_PLAIN) {
                    a = sdfk_leaf<float>(0u, C_0, PRM, TAB);
                    _Pragma("unroll 1") for (unsigned k = 1u; k < SDFK_NLEAF; ++k)
                        a = SDFK_CHAIN_CMB(a, sdfk_leaf<float>(k, C_0, PRM, TAB), PRM);
                } else {
                    a = sdfk_leaf_rec<float>(sdfk_uni(L->rec[off]), C_0, PRM, TAB);
                    _Pragma("unroll 1") for (unsigned i = 1u; i < cnt; ++i)
                        a = SDFK_CHAIN_CMB(a, sdfk_leaf_rec<float>(sdfk_uni(L->rec[off + i]), C_0, PRM, TAB), PRM);
                }
                acc = a;
            }
        }
        return sdfk_chain_tail<float>(acc, C_0, PRM, TAB);
    }
};

// the field of a culled kernel (SDFK_MARCH_KERNEL, sdfk_raydev.h): one set of lists per wave of the workgroup
#define SDFK_FIELD_CULL                                   \
    __shared__ sdfk_raylists lists[SDFK_RAY_BLOCK / 64]; \
    const SdfkCullField field = {PRM, TAB, &lists[sdfk_tx() >> 6], STATS, (int)(sdfk_tx() & 63u), {0.0f, 0.0f, 0.0f}, -1.0f, 0u, 0u}

#endif  // SDFK_RAYCULL_H
