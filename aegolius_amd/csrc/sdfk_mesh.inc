// sdfk_mesh.inc — isosurface (3-D) and contour (2-D) extraction from a field resident in HBM (included by sdfk.hip after
// sdfk_fieldops.inc, whose selection count kernel and scan it reuses).
//
// Output definition: aegolius_amd/mesh.py and DESIGN §4.13. A point is inside if field <= level (NaN outside: the key
// of sdfk_sel_key, the rule of sdfk_field_select). Point p owns the grid edges to p + s_a (axis a, stride s_a); a
// vertex sits on every owned edge whose two ends differ, numbered by (p, a). A cell is named by its minimum corner;
// its triangles (segments in 2-D) come from the generated case table (sdfk_mesh_table.inc, aegolius_amd/_mctable.py)
// and are numbered by (cell, table order).
//
// Passes over a tile of 8192 points (256 words of 32 inside bits, one word per thread):
//   bits   sdfk_select_count_kernel<true>: the field read once, 4 B/point, one bit per point out (the selection's pass)
//   count  from the bits alone: per word the crossing bits of the owned edges (neighbour bits by funnel shifts of the
//          bit string), the cell cases of the "mixed" cells (some corners inside, some not) and their triangle counts;
//          per tile the totals, per word the in-tile prefixes. Tiles with any output keep the word records.
//   scan   sdfk_select_scan_kernel, once over the tile vertex counts, once over the triangle counts
//   emit   tiles without output leave at once. Vertices: sparse field reads at the crossing edges. Triangle corners:
//          vertex id = tile offset + word prefix + popcount of the crossing bits below the edge's owner point.
//          Plain stores, no atomics: the order is the definition's.
// Point, vertex and face indices are 64-bit; faces are stored as 32-bit when the caller asks for it (V < 2^31).

#include "sdfk_mesh_table.inc"

#define SDFK_MESH_THREADS SDFK_SEL_THREADS        // words per tile: the selection's tile of 8192 points

struct MeshGeom {
    long long n;          // points
    long long words;      // words of the bit string: tiles * 256
    long long s[3];       // axis strides (2-D: s[0], s[1])
    long long rowlen;     // points per row (the fastest axis)
    int d[3];             // axis lengths (2-D: d[0], d[1])
};

// the 32 inside bits of points p .. p + 31 (p >= 0); zeros past the bit string
static __device__ __forceinline__ unsigned mesh_bits_at(const unsigned* __restrict__ bits, long long words, long long p) {
    const long long q = p >> 5;
    const unsigned r = (unsigned)p & 31u;
    const unsigned lo = q < words ? bits[q] : 0u;
    const unsigned hi = q + 1 < words ? bits[q + 1] : 0u;
    return r ? (lo >> r) | (hi << (32u - r)) : lo;
}

static __device__ __forceinline__ unsigned mesh_span(long long lo, long long hi) {     // bits [lo, hi) of a word
    return (unsigned)(((1ull << hi) - 1ull) & ~((1ull << lo) - 1ull));
}

// valid[a]: bits of the word at p0 whose point has a successor along axis a (and lies in the grid)
template <int D>
static __device__ __forceinline__ void mesh_valid(const MeshGeom& g, long long p0, unsigned* valid) {
    const long long end = p0 + 32 < g.n ? p0 + 32 : g.n;
    unsigned last = 0, rowbad = 0, planebad = 0, in = 0;
    if (p0 < end) {
        long long r = p0 / g.rowlen, rs = r * g.rowlen;
        long long j = D == 3 ? r % g.d[1] : r, i = D == 3 ? r / g.d[1] : 0;   // (3-D: row r = (i, j); 2-D: row r = i)
        for (; rs < end; ++r, rs += g.rowlen) {
            const long long lo = rs > p0 ? rs - p0 : 0, hi = (rs + g.rowlen < end ? rs + g.rowlen : end) - p0;
            const unsigned seg = mesh_span(lo, hi);
            in |= seg;
            const long long tail = rs + g.rowlen - 1 - p0;
            if (tail < 32) last |= 1u << tail;
            if (D == 3) {
                if (j == g.d[1] - 1) rowbad |= seg;
                if (i == g.d[0] - 1) planebad |= seg;
                if (++j == g.d[1]) {
                    j = 0;
                    ++i;
                }
            } else {
                if (j == g.d[0] - 1) rowbad |= seg;
                ++j;
            }
        }
    }
    if (D == 3) {
        valid[0] = in & ~planebad;
        valid[1] = in & ~rowbad;
        valid[2] = in & ~last;
    } else {
        valid[0] = in & ~rowbad;
        valid[1] = in & ~last;
        valid[2] = 0;
    }
}

// inside bits of the 2^D cell corners of the word's 32 cells (corner c: offsets from its bits, _mctable.py numbering)
template <int D>
static __device__ __forceinline__ void mesh_corners(const unsigned* __restrict__ bits, const MeshGeom& g, long long p0,
                                                    unsigned b0, unsigned* k) {
    k[0] = b0;
#pragma unroll
    for (int c = 1; c < (1 << D); ++c) {
        long long off = 0;
#pragma unroll
        for (int a = 0; a < D; ++a)
            if (c >> (D - 1 - a) & 1) off += g.s[a];
        k[c] = mesh_bits_at(bits, g.words, p0 + off);
    }
}

// cells of the word with some corners inside and some outside
template <int D>
static __device__ __forceinline__ unsigned mesh_mixed(const unsigned* k, const unsigned* valid) {
    unsigned all = k[0], any = k[0];
#pragma unroll
    for (int c = 1; c < (1 << D); ++c) {
        all &= k[c];
        any |= k[c];
    }
    unsigned cell = valid[0] & valid[1];
    if (D == 3) cell &= valid[2];
    return any & ~all & cell;
}

template <int D>
static __device__ __forceinline__ unsigned mesh_case(const unsigned* k, int b) {
    unsigned cs = 0;
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) cs |= ((k[c] >> b) & 1u) << c;
    return cs;
}

static __device__ __forceinline__ unsigned mesh_block_exclusive(unsigned v, unsigned* total, unsigned* wsum) {
    const int lane = sdfk_tx() & 63, wave = sdfk_tx() >> 6;
    const int incl = sdfk_wave_inclusive((int)v, lane);
    if (lane == 63) wsum[wave] = (unsigned)incl;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int w = 0; w < SDFK_MESH_THREADS / 64; ++w) {
        before += w < wave ? wsum[w] : 0u;
        all += wsum[w];
    }
    *total = all;
    return before + (unsigned)incl - v;
}

// count pass: one word per thread, one tile per workgroup
template <int D>
__global__ __launch_bounds__(SDFK_MESH_THREADS) void sdfk_mesh_count_kernel(const unsigned* __restrict__ bits, MeshGeom g,
                                                                            unsigned long long* __restrict__ vblk,
                                                                            unsigned long long* __restrict__ tblk,
                                                                            uint4* __restrict__ rec, unsigned* __restrict__ tpre) {
    __shared__ unsigned wsum[2][SDFK_MESH_THREADS / 64];
    const long long w = (long long)sdfk_bx() * SDFK_MESH_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    const unsigned b0 = bits[w];
    unsigned valid[3], cross[3] = {0u, 0u, 0u}, k[1 << D];
    mesh_valid<D>(g, p0, valid);
    mesh_corners<D>(bits, g, p0, b0, k);
    // the owned edges' far ends are corners 4, 2, 1 (3-D) / 2, 1 (2-D)
#pragma unroll
    for (int a = 0; a < D; ++a) cross[a] = (b0 ^ k[1 << (D - 1 - a)]) & valid[a];
    unsigned mixed = mesh_mixed<D>(k, valid), nt = 0;
    while (mixed) {
        const int b = __builtin_ctz(mixed);
        mixed &= mixed - 1u;
        const unsigned cs = mesh_case<D>(k, b);
        nt += D == 3 ? sdfk_mc_ntri[cs] : sdfk_ms_nseg[cs];
    }
    const unsigned nv = __popc(cross[0]) + __popc(cross[1]) + __popc(cross[2]);
    unsigned vtot, ttot;
    const unsigned vp = mesh_block_exclusive(nv, &vtot, wsum[0]);
    const unsigned tp = mesh_block_exclusive(nt, &ttot, wsum[1]);
    if (vtot | ttot) {                                         // block-uniform: the emit pass reads these tiles only
        rec[w] = make_uint4(cross[0], cross[1], cross[2], vp);
        tpre[w] = tp;
    }
    if (sdfk_tx() == 0) {
        vblk[sdfk_bx()] = vtot;
        tblk[sdfk_bx()] = ttot;
    }
}

// vertex id of the edge (owner point q, axis a): its tile's offset + its word's prefix + the crossings below it
static __device__ __forceinline__ long long mesh_vertex_id(const uint4* __restrict__ rec, const unsigned long long* __restrict__ vblk,
                                                           long long q, int a) {
    const long long w = q >> 5;
    const unsigned r = (unsigned)q & 31u, below = (1u << r) - 1u;
    const uint4 R = rec[w];
    long long id = (long long)vblk[w / SDFK_MESH_THREADS] + R.w + __popc(R.x & below) + __popc(R.y & below) + __popc(R.z & below);
    if (a > 0) id += (R.x >> r) & 1u;
    if (a > 1) id += (R.y >> r) & 1u;
    return id;
}

static __device__ __forceinline__ bool mesh_isnan(float v) {
    return (__builtin_bit_cast(unsigned, v) & 0x7fffffffu) > 0x7f800000u;
}

// the vertex coordinate on an edge from xa (value fa) to xb (value fb): the definition's arithmetic and NaN rules, ONE
// function for both paths (the field emit and the placement of the geometry path), so that they cannot drift apart
static __device__ __forceinline__ float mesh_place(float fa, float fb, float xa, float xb, float level) {
    if (mesh_isnan(fa)) return xb;
    if (mesh_isnan(fb)) return xa;
    const float t = (level - fa) / (fb - fa);
    return xa + t * (xb - xa);
}

// ENDS = false: the vertices from the field. ENDS = true (geometry path, f unused): for vertex v the coordinates of its
// edge's two ends go to columns 2 v (lower end) and 2 v + 1 of the (3, es) array vout — z = 0 in 2-D —, to be evaluated
// and placed afterwards (sdfk_mesh_place_kernel). Triangles are the same in both.
template <int D, typename IDX, bool ENDS>
__global__ __launch_bounds__(SDFK_MESH_THREADS) void sdfk_mesh_emit_kernel(const float* __restrict__ f, const unsigned* __restrict__ bits,
                                                                           MeshGeom g, const float* __restrict__ axes, float level,
                                                                           const unsigned long long* __restrict__ vblk,
                                                                           const unsigned long long* __restrict__ tblk,
                                                                           const uint4* __restrict__ rec,
                                                                           const unsigned* __restrict__ tpre,
                                                                           float* __restrict__ vout, long long vcap, long long es,
                                                                           IDX* __restrict__ fout, long long fcap) {
    const long long tile = sdfk_bx();
    if (vblk[tile + 1] == vblk[tile] && tblk[tile + 1] == tblk[tile]) return;
    const long long w = tile * SDFK_MESH_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    const uint4 R = rec[w];
    // vertices, in (point, axis) order
    long long vid = (long long)vblk[tile] + R.w;
    const unsigned cross[3] = {R.x, R.y, R.z};
    unsigned any = R.x | R.y | R.z;
    while (any) {
        const int b = __builtin_ctz(any);
        any &= any - 1u;
        const long long p = p0 + b;
        long long idx[3];
        if (D == 3) {
            idx[0] = p / g.s[0];
            const long long rem = p - idx[0] * g.s[0];
            idx[1] = rem / g.s[1];
            idx[2] = rem - idx[1] * g.s[1];
        } else {
            idx[0] = p / g.s[0];
            idx[1] = p - idx[0] * g.s[0];
            idx[2] = 0;
        }
        const float* ax[3] = {axes, axes + g.d[0], axes + g.d[0] + g.d[1]};
        float base[3];
#pragma unroll
        for (int o = 0; o < D; ++o) base[o] = ax[o][idx[o]];
#pragma unroll
        for (int a = 0; a < D; ++a) {
            if (!(cross[a] >> b & 1u)) continue;
            const float xa = base[a], xb = ax[a][idx[a] + 1];
            if (vid < vcap) {
                if (ENDS) {
#pragma unroll
                    for (int o = 0; o < 3; ++o) {
                        const float lo = o < D ? base[o] : 0.0f;
                        *reinterpret_cast<float2*>(vout + o * es + 2 * vid) = make_float2(lo, o == a ? xb : lo);
                    }
                } else {
                    const float x = mesh_place(f[p], f[p + g.s[a]], xa, xb, level);
                    float* dst = vout + vid * D;
#pragma unroll
                    for (int o = 0; o < D; ++o) dst[o] = o == a ? x : base[o];
                }
            }
            ++vid;
        }
    }
    // triangles (segments), in (cell, table) order
    long long fid = (long long)tblk[tile] + tpre[w];
    unsigned valid[3], k[1 << D];
    mesh_valid<D>(g, p0, valid);
    mesh_corners<D>(bits, g, p0, bits[w], k);
    unsigned mixed = mesh_mixed<D>(k, valid);
    while (mixed) {
        const int b = __builtin_ctz(mixed);
        mixed &= mixed - 1u;
        const long long p = p0 + b;
        const unsigned cs = mesh_case<D>(k, b);
        const int ne = D == 3 ? 3 * sdfk_mc_ntri[cs] : 2 * sdfk_ms_nseg[cs];
        const unsigned char* tab = D == 3 ? sdfk_mc_tri[cs] : sdfk_ms_seg[cs];
        for (int e = 0; e < ne; ++e) {
            const int edge = tab[e];
            // edge -> (axis, owner point): 3-D e = 4 a + (u << 1 | v) over the two other axes; 2-D e = 2 a + u
            int a;
            long long q = p;
            if (D == 3) {
                a = edge >> 2;
                const int o1 = a == 0 ? 1 : 0, o2 = a == 2 ? 1 : 2;
                if (edge & 2) q += g.s[o1];
                if (edge & 1) q += g.s[o2];
            } else {
                a = edge >> 1;
                if (edge & 1) q += g.s[1 - a];
            }
            const long long id = mesh_vertex_id(rec, vblk, q, a);
            if (fid < fcap) fout[fid * D + e % D] = (IDX)id;
            if (e % D == D - 1) ++fid;
        }
    }
}

// ---- geometry path (no field): evaluate -> flags -> bits, count and scan as above, emit edge ends -> evaluate -> place ----
// flags -> bits: the brick-tiled slots of the evaluation's flag build (sdfk_fieldops.inc, "fused selection") into the linear
// bit string. One output word per thread: word w (points 32 w .. 32 w + 31) ORs the slot of every row that has points in
// it — at most two, rows have >= 32 points. Words past n, and slots outside the rows' windows, are zeros.
__global__ __launch_bounds__(SDFK_MESH_THREADS) void sdfk_mesh_flags_bits_kernel(const unsigned* __restrict__ flags, SelGeom sg,
                                                                                 long long n, unsigned* __restrict__ bits) {
    const long long w = (long long)sdfk_bx() * SDFK_MESH_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    unsigned out = 0u;
    if (p0 < n) {
        const long long r1 = (p0 + 31 < n ? p0 + 31 : n - 1) / sg.L;
        for (long long r = p0 / sg.L; r <= r1 && r < sg.R; ++r) {
            const long long k = w - ((r * sg.L) >> 5);
            if (k >= 0 && k < (long long)sg.nchunk) out |= flags[((r / sg.RB) * sg.nchunk + k) * sg.RB + r % sg.RB];
        }
    }
    bits[w] = out;
}

// vertex v from its edge's two ends (columns 2 v, 2 v + 1 of the (3, es) array `ends`) and their values: along the one
// axis where the ends differ, mesh_place; elsewhere the shared coordinate
template <int D>
__global__ __launch_bounds__(256) void sdfk_mesh_place_kernel(const float* __restrict__ ends, long long es, const float* __restrict__ vals,
                                                              long long nv, float level, float* __restrict__ vout, long long step) {
    for (long long v = (long long)sdfk_bx() * 256 + sdfk_tx(); v < nv; v += step) {
        const float2 fv = *reinterpret_cast<const float2*>(vals + 2 * v);
        float x[D];
#pragma unroll
        for (int o = 0; o < D; ++o) {
            const float2 e = *reinterpret_cast<const float2*>(ends + o * es + 2 * v);
            x[o] = e.x == e.y ? e.x : mesh_place(fv.x, fv.y, e.x, e.y, level);
        }
#pragma unroll
        for (int o = 0; o < D; ++o) vout[v * D + o] = x[o];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// scratch: vblk (tiles + 1) u64 | tblk (tiles + 1) u64 | axis tables | bit string (words u32) | records (words uint4) |
// triangle prefixes (words u32); regions 256-byte aligned. The geometry path's flag slots live in the record region
// (rec_min: their bytes, when they could need more than it has) until the count pass overwrites it.
struct MeshScratch {
    unsigned long long* vblk;
    unsigned long long* tblk;
    float* axes;
    unsigned* bits;
    uint4* rec;
    unsigned* tpre;
    long long tiles;
};
static size_t mesh_align(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t mesh_layout(long long n, long long naxis, MeshScratch* sc, void* base, size_t rec_min = 0) {
    const long long tiles = (n + SDFK_SEL_TILE - 1) / SDFK_SEL_TILE;
    const long long words = tiles * SDFK_MESH_THREADS;
    size_t off = 0;
    size_t o_v = off; off += mesh_align((size_t)(tiles + 1) * 8);
    size_t o_t = off; off += mesh_align((size_t)(tiles + 1) * 8);
    size_t o_a = off; off += mesh_align((size_t)naxis * 4);
    size_t o_b = off; off += mesh_align((size_t)words * 4);
    size_t o_r = off; off += mesh_align(std::max((size_t)words * 16, rec_min));
    size_t o_p = off; off += mesh_align((size_t)words * 4);
    if (sc) {
        char* c = static_cast<char*>(base);
        sc->vblk = reinterpret_cast<unsigned long long*>(c + o_v);
        sc->tblk = reinterpret_cast<unsigned long long*>(c + o_t);
        sc->axes = reinterpret_cast<float*>(c + o_a);
        sc->bits = reinterpret_cast<unsigned*>(c + o_b);
        sc->rec = reinterpret_cast<uint4*>(c + o_r);
        sc->tpre = reinterpret_cast<unsigned*>(c + o_p);
        sc->tiles = tiles;
    }
    return off;
}

static int mesh_geom(int D, const int64_t* dims, MeshGeom* g, const char* who) {
    long long n = 1;
    for (int a = 0; a < D; ++a) {
        if (dims[a] < 2 || dims[a] > 0x3fffffff) return fail(-1, std::string(who) + ": every axis needs 2 to 2^30 points");
        n *= dims[a];
        if (n > (1ll << 46)) return fail(-1, std::string(who) + ": grid too large");
    }
    g->n = n;
    g->words = (n + SDFK_SEL_TILE - 1) / SDFK_SEL_TILE * SDFK_MESH_THREADS;
    g->d[0] = (int)dims[0];
    g->d[1] = (int)dims[1];
    g->d[2] = D == 3 ? (int)dims[2] : 1;
    if (D == 3) {
        g->s[0] = dims[1] * dims[2];
        g->s[1] = dims[2];
        g->s[2] = 1;
        g->rowlen = dims[2];
    } else {
        g->s[0] = dims[1];
        g->s[1] = 1;
        g->s[2] = 0;
        g->rowlen = dims[1];
    }
    // (the per-tile kernels launch tiles x SDFK_MESH_THREADS work-items: fewer than 2^32)
    if (g->words > 0xffffffffll) return fail(-1, std::string(who) + ": grid too large");
    return 0;
}

static bool mesh_level_ok(float level) { return sdfk_sel_key(level) != 0xffffffffu; }

// where the inside bits come from: a resident field, or (geometry path) a program evaluated on the grid of the axis tables
struct MeshSrc {
    const float* field;
    sdfk_program* prog;
    int mode;
};

// the geometry path's grid: rows along the last axis longer than one point, as plan_eval and sdfk_eval_grid_select take them
static long long mesh_grow(int D, const int64_t* dims) { return D == 3 ? dims[2] : dims[1]; }
// bytes of the brick-tiled flag slots the evaluation may write, with the padding select_prepare clears (0: rows too short
// for the row-block kernels, whose flags are the linear bit string itself)
static size_t mesh_flag_bytes(int D, const int64_t* dims, long long n) {
    const long long grow = mesh_grow(D, dims);
    if (grow < 32) return 0;
    return (size_t)(sel_words(sel_geom(n, grow, true)) + 64) * sizeof(unsigned);
}
// axis floats in the scratch: the tables, and for a 2-D geometry the third axis (the single 0.0 of a flat grid)
static long long mesh_naxis(int D, const int64_t* dims, bool geo) {
    long long naxis = 0;
    for (int a = 0; a < D; ++a) naxis += dims[a];
    return naxis + (geo && D == 2 ? 1 : 0);
}
static void mesh_scratch(int D, const int64_t* dims, const MeshGeom& g, const MeshSrc& src, void* d_scratch, MeshScratch* sc) {
    mesh_layout(g.n, mesh_naxis(D, dims, src.prog != nullptr), sc, d_scratch, src.prog ? mesh_flag_bytes(D, dims, g.n) : 0);
}

// geometry path, bits pass: the flag builds of the evaluation kernels (the specialised plain / row-block kernels only, as the
// fused selection) write one inside bit per point with the mesh's key, sdfk_sel_key(f) <= sdfk_sel_key(level). Linear
// layout: straight into the bit string. Brick-tiled layout: into the record region, then sdfk_mesh_flags_bits_kernel.
template <int D>
static int mesh_eval_bits(const MeshSrc& src, const int64_t* dims, const MeshGeom& g, const MeshScratch& sc, float level,
                          hipStream_t stream, const char* who) {
    const long long grow = mesh_grow(D, dims), rows = g.n / grow;
    // Slabs of whole rows, at most 2^32 points each: a launch holds fewer than 2^32 work-items (the row-block kernel's
    // tiles x threads passed that at 4097^3, and the plain kernel's n / 4 from 2^34 points on). A slab starts at a
    // multiple of 32 rows, so that its flags are the global ones shifted by whole words: brick-tiled, blocks of 16 rows
    // (row0 * nchunk words); linear, row0 * grow / 32 words. (The layout is that of every slab: the first is the largest.)
    const long long slab = std::max(32ll, ((1ll << 32) / grow) & ~31ll);
    if (slab * grow > (1ll << 32)) return fail(-1, std::string(who) + ": rows longer than 2^27 points");
    SrcGrid grid;
    grid.ax0 = sc.axes;
    grid.ax1 = sc.axes + dims[0];
    grid.ax2 = sc.axes + dims[0] + dims[1];                    // (2-D: the 0.0 behind the two tables)
    grid.n1 = (unsigned)dims[1];
    grid.n2 = D == 3 ? (unsigned)dims[2] : 1u;
    grid.start = 0;
    EvalCall c = grid_call(src.prog, &grid, std::min(slab, rows) * grow, nullptr, stream, src.mode, true);
    c.d_flags = sc.bits;                                       // (the planner asks whether flags are written; where is set per slab)
    c.thr_key = sdfk_sel_key(level);
    EvalPlan first;                                            // the layout is that of every slab: the first is the largest
    int rc = plan_eval(c, plan_env(), &first);
    if (rc) return rc;
    const bool tiled = first.rows();
    const SelGeom sg = sel_geom(g.n, grow, tiled);
    unsigned* flags = tiled ? reinterpret_cast<unsigned*>(sc.rec) : sc.bits;
    if (tiled) HIPCHK(hipMemsetAsync(flags + sel_words(sg), 0, 64 * sizeof(unsigned), stream));
    else HIPCHK(hipMemsetAsync(sc.bits, 0, (size_t)g.words * sizeof(unsigned), stream));
    for (long long row0 = 0; row0 < rows; row0 += slab) {
        c.n = std::min(slab, rows - row0) * grow;
        grid.start = row0 * grow;
        c.d_flags = flags + (tiled ? row0 * (long long)sg.nchunk : row0 * grow / 32);
        rc = run(c);
        if (rc) return rc;
    }
    if (tiled)
        hipLaunchKernelGGL(sdfk_mesh_flags_bits_kernel, dim3((unsigned)(g.words / SDFK_MESH_THREADS)), dim3(SDFK_MESH_THREADS), 0, stream,
                           flags, sg, g.n, sc.bits);
    return 0;
}

template <int D>
static int mesh_count(const MeshSrc& src, const float* const* ax, const int64_t* dims, float level, int64_t* nv, int64_t* nf,
                      void* d_scratch, void* stream_, const char* who) {
    if (!nv || !nf || !(src.field || src.prog) || !d_scratch) return fail(-1, std::string(who) + ": bad arguments");
    *nv = *nf = 0;
    if ((uintptr_t)src.field & 15) return fail(-1, std::string(who) + ": the field must be 16-byte aligned");
    if ((uintptr_t)d_scratch & 255) return fail(-1, std::string(who) + ": the scratch must be 256-byte aligned");
    if (src.prog && src.prog->n_aux > 0)
        return fail(-1, std::string(who) + ": staged programs (auxiliary fields) are evaluated to a field first");
    if (!mesh_level_ok(level)) return fail(-1, std::string(who) + ": the level is NaN");
    MeshGeom g;
    int rc = mesh_geom(D, dims, &g, who);
    if (rc) return rc;
    for (int a = 0; a < D; ++a) {
        if (!ax[a]) return fail(-1, std::string(who) + ": axis table missing");
        for (long long i = 0; i + 1 < dims[a]; ++i)
            if (!(ax[a][i] < ax[a][i + 1])) return fail(-1, std::string(who) + ": axis tables must be strictly increasing");
    }
    MeshScratch sc;
    mesh_scratch(D, dims, g, src, d_scratch, &sc);
    hipStream_t stream = (hipStream_t)stream_;
    long long at = 0;
    for (int a = 0; a < D; ++a) {
        HIPCHK(hipMemcpyAsync(sc.axes + at, ax[a], (size_t)dims[a] * sizeof(float), hipMemcpyHostToDevice, stream));
        at += dims[a];
    }
    const long long nb = sc.tiles;
    if (src.prog) {
        if (D == 2) HIPCHK(hipMemsetAsync(sc.axes + at, 0, sizeof(float), stream));
        rc = mesh_eval_bits<D>(src, dims, g, sc, level, stream, who);
        if (rc) return rc;
    } else {
        // bits pass: the selection's count kernel (its per-tile counts land in vblk and are overwritten by the count pass)
        hipLaunchKernelGGL(sdfk_select_count_kernel<true>, dim3((unsigned)((nb + SDFK_SEL_TPW - 1) / SDFK_SEL_TPW)), dim3(SDFK_SEL_THREADS),
                           0, stream, src.field, g.n, sdfk_sel_key(level), sc.vblk, sc.bits);
    }
    hipLaunchKernelGGL(sdfk_mesh_count_kernel<D>, dim3((unsigned)nb), dim3(SDFK_MESH_THREADS), 0, stream, sc.bits, g, sc.vblk, sc.tblk,
                       sc.rec, sc.tpre);
    hipLaunchKernelGGL(sdfk_select_scan_kernel, dim3(1), dim3(1024), 0, stream, sc.vblk, nb);
    hipLaunchKernelGGL(sdfk_select_scan_kernel, dim3(1), dim3(1024), 0, stream, sc.tblk, nb);
    hipError_t e = hipGetLastError();
    unsigned long long tot[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&tot[0], sc.vblk + nb, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&tot[1], sc.tblk + nb, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    *nv = (int64_t)tot[0];
    *nf = (int64_t)tot[1];
    return 0;
}

template <int D, typename IDX>
static void mesh_emit(const MeshSrc& src, const MeshGeom& g, const MeshScratch& sc, float level, float* vout, long long vcap,
                      long long es, void* d_faces, long long fcap, hipStream_t stream) {
    const dim3 grid((unsigned)sc.tiles), block(SDFK_MESH_THREADS);
    if (src.prog)
        hipLaunchKernelGGL((sdfk_mesh_emit_kernel<D, IDX, true>), grid, block, 0, stream, static_cast<const float*>(nullptr), sc.bits, g,
                           sc.axes, level, sc.vblk, sc.tblk, sc.rec, sc.tpre, vout, vcap, es, static_cast<IDX*>(d_faces), fcap);
    else
        hipLaunchKernelGGL((sdfk_mesh_emit_kernel<D, IDX, false>), grid, block, 0, stream, src.field, sc.bits, g, sc.axes, level,
                           sc.vblk, sc.tblk, sc.rec, sc.tpre, vout, vcap, es, static_cast<IDX*>(d_faces), fcap);
}

template <int D>
static int mesh_finish(const MeshSrc& src, const int64_t* dims, float level, int64_t nv, int64_t nf, float* d_vertices,
                       int64_t vcap, void* d_faces, int64_t fcap, int face_bytes, void* d_scratch, void* stream_,
                       const char* who) {
    if (!(src.field || src.prog) || !d_scratch || ((uintptr_t)d_scratch & 255) || nv < 0 || nf < 0 || (face_bytes != 4 && face_bytes != 8))
        return fail(-1, std::string(who) + ": bad arguments");
    if (src.prog && src.prog->n_aux > 0)
        return fail(-1, std::string(who) + ": staged programs (auxiliary fields) are evaluated to a field first");
    if (!mesh_level_ok(level)) return fail(-1, std::string(who) + ": the level is NaN");
    if (nv > vcap || nf > fcap || (nv && !d_vertices) || (nf && !d_faces))
        return fail(-1, std::string(who) + ": output buffers smaller than the mesh");
    if (face_bytes == 4 && nv > 0x7fffffffll) return fail(-1, std::string(who) + ": 32-bit faces need fewer than 2^31 vertices");
    MeshGeom g;
    int rc = mesh_geom(D, dims, &g, who);
    if (rc) return rc;
    MeshScratch sc;
    mesh_scratch(D, dims, g, src, d_scratch, &sc);
    const long long nb = sc.tiles;
    unsigned long long tot[2] = {0, 0};
    HIPCHK(hipMemcpy(&tot[0], sc.vblk + nb, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&tot[1], sc.tblk + nb, 8, hipMemcpyDeviceToHost));
    if ((int64_t)tot[0] != nv || (int64_t)tot[1] != nf)
        return fail(-1, std::string(who) + ": the scratch does not hold a mesh of that size");
    if (nv == 0 && nf == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    // geometry path: the edge ends (3 rows of es floats) and their values (es floats), 16 * es bytes for the mesh's lifetime
    const long long es = src.prog ? (2 * nv + 63) / 64 * 64 : 0;
    Scratch ends;
    if (src.prog && ends.get(nullptr, (size_t)(es > 0 ? es : 64) * 4 * sizeof(float)))
        return fail(-5, std::string(who) + ": out of device memory (edge ends)");
    float* vout = src.prog ? static_cast<float*>(ends.p) : d_vertices;
    if (face_bytes == 4) mesh_emit<D, int>(src, g, sc, level, vout, nv, es, d_faces, nf, stream);
    else mesh_emit<D, long long>(src, g, sc, level, vout, nv, es, d_faces, nf, stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && src.prog && nv > 0) {
        float* vals = static_cast<float*>(ends.p) + 3 * es;
        // the 2 V ends in chunks of 2^32 points (launch sizes, as the slabs of mesh_eval_bits); rows of es floats
        for (long long off = 0; off < 2 * nv; off += 1ll << 32) {
            SrcArray a = {static_cast<const float*>(ends.p) + off, es};
            rc = run(array_call(src.prog, &a, std::min(2 * nv - off, 1ll << 32), vals + off, stream, src.mode, true));
            if (rc) return rc;
        }
        const long long blocks = std::min<long long>((nv + 255) / 256, 1ll << 20);
        hipLaunchKernelGGL(sdfk_mesh_place_kernel<D>, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<const float*>(ends.p), es,
                           static_cast<const float*>(vals), (long long)nv, level, d_vertices, blocks * 256);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    return 0;
}

extern "C" size_t sdfk_field_isosurface_scratch(int64_t n0, int64_t n1, int64_t n2) {
    if (n0 < 1 || n1 < 1 || n2 < 1) return 256;
    return mesh_layout(n0 * n1 * n2, n0 + n1 + n2, nullptr, nullptr);
}
extern "C" int sdfk_field_isosurface(const float* d_field, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                     const float* ax2, int64_t n2, float level, int64_t* n_vertices, int64_t* n_faces,
                                     void* d_scratch, void* stream) {
    const float* ax[3] = {ax0, ax1, ax2};
    const int64_t dims[3] = {n0, n1, n2};
    return mesh_count<3>(MeshSrc{d_field, nullptr, 0}, ax, dims, level, n_vertices, n_faces, d_scratch, stream, "sdfk_field_isosurface");
}
extern "C" int sdfk_field_isosurface_finish(const float* d_field, int64_t n0, int64_t n1, int64_t n2, float level,
                                            int64_t n_vertices, int64_t n_faces, float* d_vertices, int64_t vertex_capacity,
                                            void* d_faces, int64_t face_capacity, int face_bytes, void* d_scratch, void* stream) {
    const int64_t dims[3] = {n0, n1, n2};
    return mesh_finish<3>(MeshSrc{d_field, nullptr, 0}, dims, level, n_vertices, n_faces, d_vertices, vertex_capacity, d_faces,
                          face_capacity, face_bytes, d_scratch, stream, "sdfk_field_isosurface_finish");
}
extern "C" size_t sdfk_field_contour2d_scratch(int64_t n0, int64_t n1) {
    if (n0 < 1 || n1 < 1) return 256;
    return mesh_layout(n0 * n1, n0 + n1, nullptr, nullptr);
}
extern "C" int sdfk_field_contour2d(const float* d_field, const float* ax0, int64_t n0, const float* ax1, int64_t n1, float level,
                                    int64_t* n_vertices, int64_t* n_segments, void* d_scratch, void* stream) {
    const float* ax[3] = {ax0, ax1, nullptr};
    const int64_t dims[3] = {n0, n1, 1};
    return mesh_count<2>(MeshSrc{d_field, nullptr, 0}, ax, dims, level, n_vertices, n_segments, d_scratch, stream, "sdfk_field_contour2d");
}
extern "C" int sdfk_field_contour2d_finish(const float* d_field, int64_t n0, int64_t n1, float level, int64_t n_vertices,
                                           int64_t n_segments, float* d_vertices, int64_t vertex_capacity, void* d_segments,
                                           int64_t segment_capacity, int segment_bytes, void* d_scratch, void* stream) {
    const int64_t dims[3] = {n0, n1, 1};
    return mesh_finish<2>(MeshSrc{d_field, nullptr, 0}, dims, level, n_vertices, n_segments, d_vertices, vertex_capacity, d_segments,
                          segment_capacity, segment_bytes, d_scratch, stream, "sdfk_field_contour2d_finish");
}

// ---- geometry path entry points: the same two steps, a program evaluated on the grid of the axis tables instead of a field
// The scratch holds the mesh state of the field path (0.75 B per point) with the flag slots inside its record region:
// at most 1 B per point plus O(n0 + n1 + n2 + tiles). The finish call takes the same tables, level and mode.
static size_t mesh_geo_scratch(int D, const int64_t* dims) {
    long long n = 1;
    for (int a = 0; a < D; ++a) {
        if (dims[a] < 1) return 256;
        n *= dims[a];
    }
    return mesh_layout(n, mesh_naxis(D, dims, true), nullptr, nullptr, mesh_flag_bytes(D, dims, n));
}
extern "C" size_t sdfk_eval_grid_isosurface_scratch(int64_t n0, int64_t n1, int64_t n2) {
    const int64_t dims[3] = {n0, n1, n2};
    return mesh_geo_scratch(3, dims);
}
extern "C" int sdfk_eval_grid_isosurface(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                         const float* ax2, int64_t n2, float level, int64_t* n_vertices, int64_t* n_faces,
                                         void* d_scratch, void* stream, int mode) {
    const float* ax[3] = {ax0, ax1, ax2};
    const int64_t dims[3] = {n0, n1, n2};
    if (!p) return fail(-1, "sdfk_eval_grid_isosurface: null program");
    return mesh_count<3>(MeshSrc{nullptr, p, mode}, ax, dims, level, n_vertices, n_faces, d_scratch, stream, "sdfk_eval_grid_isosurface");
}
extern "C" int sdfk_eval_grid_isosurface_finish(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                                const float* ax2, int64_t n2, float level, int64_t n_vertices, int64_t n_faces,
                                                float* d_vertices, int64_t vertex_capacity, void* d_faces, int64_t face_capacity,
                                                int face_bytes, void* d_scratch, void* stream, int mode) {
    const int64_t dims[3] = {n0, n1, n2};
    if (!p || !ax0 || !ax1 || !ax2) return fail(-1, "sdfk_eval_grid_isosurface_finish: bad arguments");
    return mesh_finish<3>(MeshSrc{nullptr, p, mode}, dims, level, n_vertices, n_faces, d_vertices, vertex_capacity, d_faces,
                          face_capacity, face_bytes, d_scratch, stream, "sdfk_eval_grid_isosurface_finish");
}
extern "C" size_t sdfk_eval_grid_contour2d_scratch(int64_t n0, int64_t n1) {
    const int64_t dims[3] = {n0, n1, 1};
    return mesh_geo_scratch(2, dims);
}
extern "C" int sdfk_eval_grid_contour2d(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1, float level,
                                        int64_t* n_vertices, int64_t* n_segments, void* d_scratch, void* stream, int mode) {
    const float* ax[3] = {ax0, ax1, nullptr};
    const int64_t dims[3] = {n0, n1, 1};
    if (!p) return fail(-1, "sdfk_eval_grid_contour2d: null program");
    return mesh_count<2>(MeshSrc{nullptr, p, mode}, ax, dims, level, n_vertices, n_segments, d_scratch, stream, "sdfk_eval_grid_contour2d");
}
extern "C" int sdfk_eval_grid_contour2d_finish(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                               float level, int64_t n_vertices, int64_t n_segments, float* d_vertices,
                                               int64_t vertex_capacity, void* d_segments, int64_t segment_capacity,
                                               int segment_bytes, void* d_scratch, void* stream, int mode) {
    const int64_t dims[3] = {n0, n1, 1};
    if (!p || !ax0 || !ax1) return fail(-1, "sdfk_eval_grid_contour2d_finish: bad arguments");
    return mesh_finish<2>(MeshSrc{nullptr, p, mode}, dims, level, n_vertices, n_segments, d_vertices, vertex_capacity, d_segments,
                          segment_capacity, segment_bytes, d_scratch, stream, "sdfk_eval_grid_contour2d_finish");
}
