// sdfk_slices.inc — plane stacks: the contours of a program on every layer of a grid (H, U, V), and their section measures
// (included by sdfk.hip after sdfk_mesh.inc, whose bit string, scan, case table, edge-end evaluation and mesh_place it
// reuses).
//
// Output definition: aegolius_amd/slices.py and DESIGN §4.22. The grid is the native one of the evaluation kernels, the
// layer its slowest axis: point p = (l nu + i) nv + j holds the program's value at (H[l], U[i], V[j]). Layer l is the
// 2-D contour of sdfk_eval_grid_contour2d on the field F[l] with axes (U, V), bit for bit; the stack's arrays are the
// layers' arrays one after the other, vertex ids global. Nothing joins two layers: a point owns its +U edge (stride
// nv) and its +V edge (stride 1) only, no +U edge and no cell in the last row of its layer, no +V edge at a row's tail.
//
// Passes (tiles of 8192 points, one word of 32 inside bits per thread, as the 3-D mesh):
//   bits     mesh_eval_bits<3>: the flag builds of the evaluation kernels, unchanged
//   count    sdfk_slice_count_kernel: crossing bits of the two in-plane axes, the 16-case squares, per-tile totals and
//            in-tile prefixes; record (cross U, cross V, 0, prefix) — the layout mesh_vertex_id reads
//   scan     sdfk_select_scan_kernel over the vertex and over the segment counts
//   offsets  sdfk_slice_offsets_kernel: one thread per layer boundary, vertices / segments owned by points below it
//   emit     sdfk_slice_emit_kernel: edge ends as grid coordinates (h, a, b), segments by mesh_vertex_id
//   place    the program at the ends (array path), then sdfk_mesh_place_kernel<2> on the (a, b) rows of the ends
//   measure  sdfk_slice_measure_kernel: one workgroup per layer, float64 sums in a fixed order, no atomics

#define SDFK_SLICE_MEASURE_THREADS 256
#define SDFK_SLICE_MEASURES 6          // area, perimeter, first moments in a and b, segments, border crossings

// corners of the word's 32 squares, the 2-D numbering of _mctable.py: bit 0 of the corner index is +V, bit 1 is +U
static __device__ __forceinline__ void slice_corners(const unsigned* __restrict__ bits, const MeshGeom& g, long long p0, unsigned b0,
                                                     unsigned* k) {
    k[0] = b0;
    k[1] = mesh_bits_at(bits, g.words, p0 + 1);
    k[2] = mesh_bits_at(bits, g.words, p0 + g.s[1]);
    k[3] = mesh_bits_at(bits, g.words, p0 + g.s[1] + 1);
}

// the word's crossing bits (cross[0]: +U edges, cross[1]: +V edges) and its mixed squares
static __device__ __forceinline__ unsigned slice_word(const unsigned* __restrict__ bits, const MeshGeom& g, long long p0, unsigned b0,
                                                      unsigned* k, unsigned* cross) {
    unsigned valid[3];
    mesh_valid<3>(g, p0, valid);                               // [1]: not the last row of its layer, [2]: not a row's tail
    slice_corners(bits, g, p0, b0, k);
    cross[0] = (b0 ^ k[2]) & valid[1];
    cross[1] = (b0 ^ k[1]) & valid[2];
    const unsigned in_plane[2] = {valid[1], valid[2]};
    return mesh_mixed<2>(k, in_plane);
}

static __device__ __forceinline__ unsigned slice_segments(const unsigned* k, unsigned mixed) {
    unsigned ns = 0;
    while (mixed) {
        const int b = __builtin_ctz(mixed);
        mixed &= mixed - 1u;
        ns += sdfk_ms_nseg[mesh_case<2>(k, b)];
    }
    return ns;
}

// count pass: one word per thread, one tile per workgroup (the record layout and rules of sdfk_mesh_count_kernel)
__global__ __launch_bounds__(SDFK_MESH_THREADS) void sdfk_slice_count_kernel(const unsigned* __restrict__ bits, MeshGeom g,
                                                                             unsigned long long* __restrict__ vblk,
                                                                             unsigned long long* __restrict__ tblk,
                                                                             uint4* __restrict__ rec, unsigned* __restrict__ tpre) {
    __shared__ unsigned wsum[2][SDFK_MESH_THREADS / 64];
    const long long w = (long long)sdfk_bx() * SDFK_MESH_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    unsigned k[4], cross[2];
    const unsigned mixed = slice_word(bits, g, p0, bits[w], k, cross);
    const unsigned ns = slice_segments(k, mixed);
    const unsigned nv = __popc(cross[0]) + __popc(cross[1]);
    unsigned vtot, stot;
    const unsigned vp = mesh_block_exclusive(nv, &vtot, wsum[0]);
    const unsigned sp = mesh_block_exclusive(ns, &stot, wsum[1]);
    if (vtot | stot) {                                         // block-uniform: later passes read these tiles only
        rec[w] = make_uint4(cross[0], cross[1], 0u, vp);
        tpre[w] = sp;
    }
    if (sdfk_tx() == 0) {
        vblk[sdfk_bx()] = vtot;
        tblk[sdfk_bx()] = stot;
    }
}

// layer offsets (after the scans): boundary l = 0 .. layers is point l nu nv; the vertices and segments owned by the
// points below it. A boundary inside a tile without output has the tile's offsets (no record was written there); the
// last one is the totals.
__global__ __launch_bounds__(256) void sdfk_slice_offsets_kernel(const unsigned* __restrict__ bits, MeshGeom g,
                                                                 const unsigned long long* __restrict__ vblk,
                                                                 const unsigned long long* __restrict__ tblk,
                                                                 const uint4* __restrict__ rec, const unsigned* __restrict__ tpre,
                                                                 long long layers, unsigned long long* __restrict__ voff,
                                                                 unsigned long long* __restrict__ soff) {
    const long long l = (long long)sdfk_bx() * 256 + sdfk_tx();
    if (l > layers) return;
    const long long tiles = g.words / SDFK_MESH_THREADS;
    if (l == layers) {
        voff[l] = vblk[tiles];
        soff[l] = tblk[tiles];
        return;
    }
    const long long p = l * g.s[0], tile = p / SDFK_SEL_TILE;
    unsigned long long v = vblk[tile], s = tblk[tile];
    if (vblk[tile + 1] != v || tblk[tile + 1] != s) {
        const long long w = p >> 5;
        const unsigned below = (1u << ((unsigned)p & 31u)) - 1u;
        const uint4 R = rec[w];
        v += R.w + __popc(R.x & below) + __popc(R.y & below);
        s += tpre[w];
        if (below) {
            unsigned k[4], cross[2];
            const unsigned mixed = slice_word(bits, g, w * 32, bits[w], k, cross);
            s += slice_segments(k, mixed & below);
        }
    }
    voff[l] = v;
    soff[l] = s;
}

// emit pass. For vertex v the grid coordinates (h, a, b) of its edge's two ends go to columns 2 v (lower end) and
// 2 v + 1 of the (3, es) array `ends`. Segments by mesh_vertex_id over the two crossing words of the record. The
// (layer, row, column) of a point is carried from the word's first point: one division by nv and one by nu per word.
template <typename IDX>
__global__ __launch_bounds__(SDFK_MESH_THREADS) void sdfk_slice_emit_kernel(const unsigned* __restrict__ bits, MeshGeom g,
                                                                            const float* __restrict__ axes,
                                                                            const unsigned long long* __restrict__ vblk,
                                                                            const unsigned long long* __restrict__ tblk,
                                                                            const uint4* __restrict__ rec,
                                                                            const unsigned* __restrict__ tpre,
                                                                            float* __restrict__ ends, long long vcap, long long es,
                                                                            IDX* __restrict__ sout, long long scap) {
    const long long tile = sdfk_bx();
    if (vblk[tile + 1] == vblk[tile] && tblk[tile + 1] == tblk[tile]) return;
    const long long w = tile * SDFK_MESH_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    const uint4 R = rec[w];
    unsigned any = R.x | R.y;
    if (any) {
        const float* H = axes;
        const float* U = axes + g.d[0];
        const float* V = U + g.d[1];
        const long long nv = g.d[2], nu = g.d[1];
        const long long row0 = p0 / nv;
        long long col = p0 - row0 * nv, l = row0 / nu, i = row0 - l * nu;
        long long vid = (long long)vblk[tile] + R.w;
        int at = 0;
        while (any) {
            const int b = __builtin_ctz(any);
            any &= any - 1u;
            col += b - at;
            at = b;
            while (col >= nv) {
                col -= nv;
                if (++i == nu) {
                    i = 0;
                    ++l;
                }
            }
            const float h = H[l], a = U[i], c = V[col];
            if (R.x >> b & 1u) {
                if (vid < vcap) {
                    *reinterpret_cast<float2*>(ends + 2 * vid) = make_float2(h, h);
                    *reinterpret_cast<float2*>(ends + es + 2 * vid) = make_float2(a, U[i + 1]);
                    *reinterpret_cast<float2*>(ends + 2 * es + 2 * vid) = make_float2(c, c);
                }
                ++vid;
            }
            if (R.y >> b & 1u) {
                if (vid < vcap) {
                    *reinterpret_cast<float2*>(ends + 2 * vid) = make_float2(h, h);
                    *reinterpret_cast<float2*>(ends + es + 2 * vid) = make_float2(a, a);
                    *reinterpret_cast<float2*>(ends + 2 * es + 2 * vid) = make_float2(c, V[col + 1]);
                }
                ++vid;
            }
        }
    }
    // segments, in (cell, table) order
    long long sid = (long long)tblk[tile] + tpre[w];
    unsigned k[4], cross[2];
    unsigned mixed = slice_word(bits, g, p0, bits[w], k, cross);
    while (mixed) {
        const int b = __builtin_ctz(mixed);
        mixed &= mixed - 1u;
        const long long p = p0 + b;
        const unsigned cs = mesh_case<2>(k, b);
        const int ne = 2 * sdfk_ms_nseg[cs];
        const unsigned char* tab = sdfk_ms_seg[cs];
        for (int e = 0; e < ne; ++e) {
            // edge -> (axis, owner point): e = 2 a + u, u the offset along the other in-plane axis
            const int edge = tab[e], a = edge >> 1;
            const long long q = p + ((edge & 1) ? (a == 0 ? 1 : g.s[1]) : 0);
            const long long id = mesh_vertex_id(rec, vblk, q, a);
            if (sid < scap) sout[sid * 2 + (e & 1)] = (IDX)id;
            if (e & 1) ++sid;
        }
    }
}

// section measures: workgroup l walks the segments [soff[l], soff[l + 1]) and the vertices [voff[l], voff[l + 1]) of
// layer l with a stride of the workgroup, every thread sums its own in that order, and the threads' sums are added by a
// fixed tree: the same bits from run to run. float64 from the float32 vertices, relative to the centre (ca, cb).
// out[6 l ..]: sum t_s / 2, sum of the lengths, sum (a0 + a1 - 2 ca) t_s / 6, the same in b, segments, vertices on the
// border of the rectangle [u0, u1] x [v0, v1].
template <typename IDX>
__global__ __launch_bounds__(SDFK_SLICE_MEASURE_THREADS) void sdfk_slice_measure_kernel(const float* __restrict__ verts,
                                                                                        const IDX* __restrict__ segs,
                                                                                        const unsigned long long* __restrict__ voff,
                                                                                        const unsigned long long* __restrict__ soff,
                                                                                        double ca, double cb, float u0, float u1,
                                                                                        float v0, float v1, double* __restrict__ out) {
    __shared__ double red[5][SDFK_SLICE_MEASURE_THREADS];
    const long long l = sdfk_bx();
    const int t = sdfk_tx();
    const long long s0 = (long long)soff[l], s1 = (long long)soff[l + 1];
    double area = 0.0, length = 0.0, ma = 0.0, mb = 0.0;
    for (long long s = s0 + t; s < s1; s += SDFK_SLICE_MEASURE_THREADS) {
        const long long i0 = (long long)segs[2 * s], i1 = (long long)segs[2 * s + 1];
        const float2 A = *reinterpret_cast<const float2*>(verts + 2 * i0);
        const float2 B = *reinterpret_cast<const float2*>(verts + 2 * i1);
        const double a0 = (double)A.x - ca, b0 = (double)A.y - cb, a1 = (double)B.x - ca, b1 = (double)B.y - cb;
        const double ts = a0 * b1 - a1 * b0;
        area += ts;
        length += hypot((double)B.x - (double)A.x, (double)B.y - (double)A.y);
        ma += (a0 + a1) * ts / 6.0;
        mb += (b0 + b1) * ts / 6.0;
    }
    double border = 0.0;                                       // (a count, exact in float64: fewer than 2^53 vertices)
    const long long e0 = (long long)voff[l], e1 = (long long)voff[l + 1];
    for (long long v = e0 + t; v < e1; v += SDFK_SLICE_MEASURE_THREADS) {
        const float2 P = *reinterpret_cast<const float2*>(verts + 2 * v);
        if (P.x == u0 || P.x == u1 || P.y == v0 || P.y == v1) border += 1.0;
    }
    red[0][t] = area;
    red[1][t] = length;
    red[2][t] = ma;
    red[3][t] = mb;
    red[4][t] = border;
    __syncthreads();
    for (int half = SDFK_SLICE_MEASURE_THREADS / 2; half > 0; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int q = 0; q < 5; ++q) red[q][t] += red[q][t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        double* o = out + SDFK_SLICE_MEASURES * l;
        o[0] = 0.5 * red[0][0];
        o[1] = red[1][0];
        o[2] = red[2][0];
        o[3] = red[3][0];
        o[4] = (double)(s1 - s0);
        o[5] = red[4][0];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// scratch: the mesh state of the 3-D geometry path on the grid (L, nu, nv) | vertex offsets (L + 1) u64 | segment offsets
struct SliceScratch {
    MeshScratch m;
    unsigned long long* voff;
    unsigned long long* soff;
};
static size_t slice_layout(const int64_t* dims, SliceScratch* sc, void* base) {
    const long long n = dims[0] * dims[1] * dims[2];
    size_t off = mesh_layout(n, dims[0] + dims[1] + dims[2], sc ? &sc->m : nullptr, base, mesh_flag_bytes(3, dims, n));
    const size_t o_v = off; off += mesh_align((size_t)(dims[0] + 1) * 8);
    const size_t o_s = off; off += mesh_align((size_t)(dims[0] + 1) * 8);
    if (sc) {
        char* c = static_cast<char*>(base);
        sc->voff = reinterpret_cast<unsigned long long*>(c + o_v);
        sc->soff = reinterpret_cast<unsigned long long*>(c + o_s);
    }
    return off;
}

// the stack's grid: L >= 1 layers of nu x nv >= 2 x 2 points (mesh_geom asks for 2 points along every axis)
static int slice_geom(const int64_t* dims, MeshGeom* g, const char* who) {
    if (dims[0] < 1 || dims[0] > 0x3fffffff) return fail(-1, std::string(who) + ": 1 to 2^30 layers");
    long long n = dims[0];
    for (int a = 1; a < 3; ++a) {
        if (dims[a] < 2 || dims[a] > 0x3fffffff) return fail(-1, std::string(who) + ": every in-plane axis needs 2 to 2^30 points");
        n *= dims[a];
        if (n > (1ll << 46)) return fail(-1, std::string(who) + ": grid too large");
    }
    g->n = n;
    g->words = (n + SDFK_SEL_TILE - 1) / SDFK_SEL_TILE * SDFK_MESH_THREADS;
    for (int a = 0; a < 3; ++a) g->d[a] = (int)dims[a];
    g->s[0] = dims[1] * dims[2];
    g->s[1] = dims[2];
    g->s[2] = 1;
    g->rowlen = dims[2];
    if (g->words > 0xffffffffll) return fail(-1, std::string(who) + ": grid too large");
    return 0;
}

static int slice_args(sdfk_program* p, const int64_t* dims, float level, void* d_scratch, MeshGeom* g, const char* who) {
    if (!p) return fail(-1, std::string(who) + ": null program");
    if (!d_scratch || ((uintptr_t)d_scratch & 255)) return fail(-1, std::string(who) + ": the scratch must be 256-byte aligned");
    if (p->n_aux > 0) return fail(-1, std::string(who) + ": staged programs (auxiliary fields) have no plane stack");
    if (!mesh_level_ok(level)) return fail(-1, std::string(who) + ": the level is NaN");
    return slice_geom(dims, g, who);
}

// counting call: tables up, evaluation to bits, count, two scans, layer offsets; the totals come back
static int slice_count(sdfk_program* p, int mode, const float* const* ax, const int64_t* dims, float level, int64_t* nv, int64_t* ns,
                       void* d_scratch, hipStream_t stream, const char* who) {
    if (!nv || !ns) return fail(-1, std::string(who) + ": bad arguments");
    *nv = *ns = 0;
    MeshGeom g;
    int rc = slice_args(p, dims, level, d_scratch, &g, who);
    if (rc) return rc;
    for (int a = 0; a < 3; ++a) {
        if (!ax[a]) return fail(-1, std::string(who) + ": axis table missing");
        for (long long i = 0; i + 1 < dims[a]; ++i)
            if (!(ax[a][i] < ax[a][i + 1])) return fail(-1, std::string(who) + ": heights and axis tables must be strictly increasing");
    }
    SliceScratch sc;
    slice_layout(dims, &sc, d_scratch);
    long long at = 0;
    for (int a = 0; a < 3; ++a) {
        HIPCHK(hipMemcpyAsync(sc.m.axes + at, ax[a], (size_t)dims[a] * sizeof(float), hipMemcpyHostToDevice, stream));
        at += dims[a];
    }
    rc = mesh_eval_bits<3>(MeshSrc{nullptr, p, mode}, dims, g, sc.m, level, stream, who);
    if (rc) return rc;
    const long long nb = sc.m.tiles, L = dims[0];
    hipLaunchKernelGGL(sdfk_slice_count_kernel, dim3((unsigned)nb), dim3(SDFK_MESH_THREADS), 0, stream, sc.m.bits, g, sc.m.vblk,
                       sc.m.tblk, sc.m.rec, sc.m.tpre);
    hipLaunchKernelGGL(sdfk_select_scan_kernel, dim3(1), dim3(1024), 0, stream, sc.m.vblk, nb);
    hipLaunchKernelGGL(sdfk_select_scan_kernel, dim3(1), dim3(1024), 0, stream, sc.m.tblk, nb);
    hipLaunchKernelGGL(sdfk_slice_offsets_kernel, dim3((unsigned)((L + 1 + 255) / 256)), dim3(256), 0, stream, sc.m.bits, g, sc.m.vblk,
                       sc.m.tblk, sc.m.rec, sc.m.tpre, L, sc.voff, sc.soff);
    hipError_t e = hipGetLastError();
    unsigned long long tot[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&tot[0], sc.voff + L, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&tot[1], sc.soff + L, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    *nv = (int64_t)tot[0];
    *ns = (int64_t)tot[1];
    return 0;
}

// emit ends, evaluate ends, place: nv vertices (a, b) to d_vertices, ns segments to d_segments; nothing is waited for.
// `ends`: 16 es bytes the caller keeps until the stream has run (es = slice_es(nv)).
static long long slice_es(int64_t nv) { return (2 * nv + 63) / 64 * 64; }
static int slice_emit(sdfk_program* p, int mode, const MeshGeom& g, const SliceScratch& sc, float level, int64_t nv, int64_t ns,
                      float* d_vertices, void* d_segments, int segment_bytes, float* ends, hipStream_t stream, const char* who) {
    if (nv == 0 && ns == 0) return 0;
    const long long es = slice_es(nv);
    const dim3 grid((unsigned)sc.m.tiles), block(SDFK_MESH_THREADS);
    if (segment_bytes == 4)
        hipLaunchKernelGGL(sdfk_slice_emit_kernel<int>, grid, block, 0, stream, sc.m.bits, g, sc.m.axes, sc.m.vblk, sc.m.tblk, sc.m.rec,
                           sc.m.tpre, ends, (long long)nv, es, static_cast<int*>(d_segments), (long long)ns);
    else
        hipLaunchKernelGGL(sdfk_slice_emit_kernel<long long>, grid, block, 0, stream, sc.m.bits, g, sc.m.axes, sc.m.vblk, sc.m.tblk,
                           sc.m.rec, sc.m.tpre, ends, (long long)nv, es, static_cast<long long*>(d_segments), (long long)ns);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    if (nv > 0) {
        float* vals = ends + 3 * es;
        for (long long off = 0; off < 2 * nv; off += 1ll << 32) {      // (launch sizes, as mesh_finish)
            SrcArray a = {ends + off, es};
            const int rc = run(array_call(p, &a, std::min(2 * (long long)nv - off, 1ll << 32), vals + off, stream, mode, true));
            if (rc) return rc;
        }
        // the in-plane rows of the ends: (a, b) are rows 1 and 2
        const long long blocks = std::min<long long>((nv + 255) / 256, 1ll << 20);
        hipLaunchKernelGGL(sdfk_mesh_place_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<const float*>(ends + es),
                           es, static_cast<const float*>(vals), (long long)nv, level, d_vertices, blocks * 256);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    }
    return 0;
}

// the totals the scratch holds against the caller's, and the offsets to the host
static int slice_offsets_out(const SliceScratch& sc, long long L, int64_t nv, int64_t ns, int64_t* vertex_offsets,
                             int64_t* segment_offsets, const char* who) {
    static_assert(sizeof(int64_t) == sizeof(unsigned long long), "offsets are copied as they are");
    HIPCHK(hipMemcpy(vertex_offsets, sc.voff, (size_t)(L + 1) * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(segment_offsets, sc.soff, (size_t)(L + 1) * 8, hipMemcpyDeviceToHost));
    if (vertex_offsets[L] != nv || segment_offsets[L] != ns)
        return fail(-1, std::string(who) + ": the scratch does not hold a stack of that size");
    return 0;
}

extern "C" size_t sdfk_eval_grid_slices_scratch(int64_t layers, int64_t nu, int64_t nv) {
    if (layers < 1 || nu < 1 || nv < 1) return 256;
    const int64_t dims[3] = {layers, nu, nv};
    return slice_layout(dims, nullptr, nullptr);
}

extern "C" int sdfk_eval_grid_slices(sdfk_program* p, const float* heights, int64_t layers, const float* u, int64_t nu,
                                     const float* v, int64_t nv, float level, int64_t* n_vertices, int64_t* n_segments,
                                     void* d_scratch, void* stream, int mode) {
    const float* ax[3] = {heights, u, v};
    const int64_t dims[3] = {layers, nu, nv};
    return slice_count(p, mode, ax, dims, level, n_vertices, n_segments, d_scratch, (hipStream_t)stream, "sdfk_eval_grid_slices");
}

extern "C" int sdfk_eval_grid_slices_finish(sdfk_program* p, int64_t layers, int64_t nu, int64_t nv, float level,
                                            int64_t n_vertices, int64_t n_segments, float* d_vertices, int64_t vertex_capacity,
                                            void* d_segments, int64_t segment_capacity, int segment_bytes,
                                            int64_t* vertex_offsets, int64_t* segment_offsets, void* d_scratch, void* stream_,
                                            int mode) {
    const char* who = "sdfk_eval_grid_slices_finish";
    const int64_t dims[3] = {layers, nu, nv};
    if (n_vertices < 0 || n_segments < 0 || (segment_bytes != 4 && segment_bytes != 8) || !vertex_offsets || !segment_offsets)
        return fail(-1, std::string(who) + ": bad arguments");
    MeshGeom g;
    int rc = slice_args(p, dims, level, d_scratch, &g, who);
    if (rc) return rc;
    if (n_vertices > vertex_capacity || n_segments > segment_capacity || (n_vertices && !d_vertices) || (n_segments && !d_segments))
        return fail(-1, std::string(who) + ": output buffers smaller than the stack");
    if (segment_bytes == 4 && n_vertices > 0x7fffffffll)
        return fail(-1, std::string(who) + ": 32-bit segments need fewer than 2^31 vertices");
    SliceScratch sc;
    slice_layout(dims, &sc, d_scratch);
    rc = slice_offsets_out(sc, layers, n_vertices, n_segments, vertex_offsets, segment_offsets, who);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    Scratch ends;                                              // edge ends and their values, for the call's lifetime
    if (ends.get(nullptr, (size_t)std::max(slice_es(n_vertices), 64ll) * 4 * sizeof(float)))
        return fail(-5, std::string(who) + ": out of device memory (edge ends)");
    rc = slice_emit(p, mode, g, sc, level, n_vertices, n_segments, d_vertices, d_segments, segment_bytes, static_cast<float*>(ends.p),
                    stream, who);
    if (rc) return rc;
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    return 0;
}

extern "C" int sdfk_eval_grid_slices_measure(sdfk_program* p, const float* heights, int64_t layers, const float* u, int64_t nu,
                                             const float* v, int64_t nv, float level, double* measures, int64_t* vertex_offsets,
                                             int64_t* segment_offsets, void* d_scratch, void* stream_, int mode) {
    const char* who = "sdfk_eval_grid_slices_measure";
    const float* ax[3] = {heights, u, v};
    const int64_t dims[3] = {layers, nu, nv};
    if (!measures || !vertex_offsets || !segment_offsets) return fail(-1, std::string(who) + ": bad arguments");
    hipStream_t stream = (hipStream_t)stream_;
    int64_t V = 0, S = 0;
    int rc = slice_count(p, mode, ax, dims, level, &V, &S, d_scratch, stream, who);
    if (rc) return rc;
    MeshGeom g;
    rc = slice_geom(dims, &g, who);
    if (rc) return rc;
    SliceScratch sc;
    slice_layout(dims, &sc, d_scratch);
    rc = slice_offsets_out(sc, layers, V, S, vertex_offsets, segment_offsets, who);
    if (rc) return rc;
    // the stack stays in memory this call owns: edge ends and values | vertices | segments | the measures
    const int sbytes = V > 0x7fffffffll ? 8 : 4;
    const size_t b_ends = mesh_align((size_t)std::max(slice_es(V), 64ll) * 4 * sizeof(float));
    const size_t b_v = mesh_align((size_t)std::max<int64_t>(V, 1) * 2 * sizeof(float));
    const size_t b_s = mesh_align((size_t)std::max<int64_t>(S, 1) * 2 * sbytes);
    const size_t b_m = (size_t)layers * SDFK_SLICE_MEASURES * sizeof(double);
    Scratch own;
    if (own.get(nullptr, b_ends + b_v + b_s + b_m)) return fail(-5, std::string(who) + ": out of device memory (the stack)");
    char* base = static_cast<char*>(own.p);
    float* d_vertices = reinterpret_cast<float*>(base + b_ends);
    void* d_segments = base + b_ends + b_v;
    double* d_measures = reinterpret_cast<double*>(base + b_ends + b_v + b_s);
    rc = slice_emit(p, mode, g, sc, level, V, S, d_vertices, d_segments, sbytes, reinterpret_cast<float*>(base), stream, who);
    if (rc) return rc;
    const double ca = 0.5 * ((double)u[0] + (double)u[nu - 1]), cb = 0.5 * ((double)v[0] + (double)v[nv - 1]);
    if (sbytes == 4)
        hipLaunchKernelGGL(sdfk_slice_measure_kernel<int>, dim3((unsigned)layers), dim3(SDFK_SLICE_MEASURE_THREADS), 0, stream, d_vertices,
                           static_cast<const int*>(d_segments), sc.voff, sc.soff, ca, cb, u[0], u[nu - 1], v[0], v[nv - 1], d_measures);
    else
        hipLaunchKernelGGL(sdfk_slice_measure_kernel<long long>, dim3((unsigned)layers), dim3(SDFK_SLICE_MEASURE_THREADS), 0, stream,
                           d_vertices, static_cast<const long long*>(d_segments), sc.voff, sc.soff, ca, cb, u[0], u[nu - 1], v[0],
                           v[nv - 1], d_measures);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(measures, d_measures, b_m, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    return 0;
}
