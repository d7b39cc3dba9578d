// sdfk_layers.inc — layer graphs of a plane stack: the components of every layer, and the links between consecutive layers
// (included by sdfk.hip after sdfk_topology.inc: it uses that file's device helpers, its scratch layout and its passes).
//
// Output definition: aegolius_amd/layers.py, include/sdfk.h and DESIGN §4.25. The grid is (layers, nu, nv), the layer the
// slowest axis; only the inside points are labelled. Two points are joined when they are in-plane neighbours of one layer
// (faces: 4, full: 8); points of different layers never are. Names and ids as in sdfk_topology.inc, so ids ascend with the
// layer. overlap(c, q), c in layer l >= 1 and q in layer l - 1: the columns (i, j) that carry c in l and q in l - 1.
//
// Passes, on the region's bit string and the scratch of the labelling:
//   label     init, compress, number and relabel of sdfk_topology.inc as they are; the merge pass is the one backward row
//             of the same layer (topo_rows' jfirst mask stops it at a layer's first row), under full with that row's left
//             and right partners
//   records   the reduce pass of sdfk_topology.inc with the in-plane border rule (its INPLANE build)
//   links     one word per thread: the word nu nv points below by funnel shift, ov = x & below under the valid-point and
//             first-layer masks. A stretch is a maximal run of set bits of ov within one grid row and one word: both labels
//             are constant in it (each side is part of one row run), so it is one candidate (label[p], label[p - nu nv],
//             length). count per word -> tile scan -> emit in word order: the candidate array does not depend on
//             scheduling. The count pass also adds the stretch lengths to supported[child], 64-bit integer adds; a wave
//             whose stretches share one child adds once.
// The candidates are combined to the sorted, unique link list on the host (layers.py): exact integer work whose result is
// defined by the sort, not by the order of emission.
// No lane waits for another lane's write; the chase and retry caps and the device error word are those of the labelling.

// the stretches of word w: ov, and the first bit of every stretch
struct LayerOverlap {
    unsigned ov, first, end;
};
static __device__ __forceinline__ LayerOverlap layer_overlap(const unsigned* __restrict__ rb, const MeshGeom& g, long long p0,
                                                             unsigned x) {
    LayerOverlap o = {0u, 0u, 0u};
    if (!x) return o;
    const TopoRows m = topo_rows<3>(g, p0);
    const unsigned ok = x & m.in & ~m.ifirst;
    if (!ok) return o;
    o.ov = ok & topo_bits_at(rb, g.words, p0 - g.s[0]);
    o.first = o.ov & ~((o.ov << 1) & ~m.start);
    o.end = m.end;
    return o;
}
// the length of the stretch that starts at bit b
static __device__ __forceinline__ int layer_stretch(const LayerOverlap& o, int b) {
    const unsigned y = o.ov >> b, e = o.end >> b;
    int len = ~y ? __builtin_ctz(~y) : 32 - b;
    if (e && __builtin_ctz(e) + 1 < len) len = __builtin_ctz(e) + 1;
    return len;
}

// merge: the union pass of sdfk_topo_merge_kernel restricted to the backward row of the same layer
template <bool FULL>
__global__ __launch_bounds__(SDFK_TOPO_THREADS) void sdfk_layer_merge_kernel(const unsigned* __restrict__ rb, MeshGeom g, int* label,
                                                                             long long cap, unsigned* err) {
    const long long w = (long long)sdfk_bx() * SDFK_TOPO_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    const unsigned x = rb[w];
    if (!x) return;
    const TopoRows m = topo_rows<3>(g, p0);
    const unsigned ok = x & m.in & ~m.jfirst;
    if (!ok) return;
    const long long q0 = p0 - g.rowlen;
    const unsigned ov = ok & topo_bits_at(rb, g.words, q0);
    topo_unions(label, ov & ~((ov << 1) & ~m.start), p0, q0, cap, err);
    if (FULL) {
        const unsigned left = ok & topo_bits_at(rb, g.words, q0 - 1) & ~m.start & ~ov;
        const unsigned right = ok & topo_bits_at(rb, g.words, q0 + 1) & ~m.end & ~ov;
        topo_unions(label, left, p0, q0 - 1, cap, err);
        topo_unions(label, right, p0, q0 + 1, cap, err);
    }
}
static void layer_launch_merge(bool full, const unsigned* rb, const MeshGeom& g, int* label, unsigned* err, unsigned tiles,
                               hipStream_t stream) {
    const long long cap = g.n;
    if (full)
        hipLaunchKernelGGL(sdfk_layer_merge_kernel<true>, dim3(tiles), dim3(SDFK_TOPO_THREADS), 0, stream, rb, g, label, cap, err);
    else
        hipLaunchKernelGGL(sdfk_layer_merge_kernel<false>, dim3(tiles), dim3(SDFK_TOPO_THREADS), 0, stream, rb, g, label, cap, err);
}

// links, count: the stretches per word (in-tile prefix to `pre`, per-tile total to `blk`), and supported[child] += length.
// A label that is no id below K raises TOPO_ERR_ID and is never used as an index.
__global__ __launch_bounds__(SDFK_TOPO_THREADS) void sdfk_layer_count_kernel(const unsigned* __restrict__ rb, const int* __restrict__ label,
                                                                             MeshGeom g, long long K, unsigned long long* __restrict__ blk,
                                                                             unsigned* __restrict__ pre,
                                                                             unsigned long long* __restrict__ supported, unsigned* err) {
    __shared__ unsigned wsum[SDFK_TOPO_THREADS / 64];
    const long long w = (long long)sdfk_bx() * SDFK_TOPO_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    const LayerOverlap o = layer_overlap(rb, g, p0, rb[w]);
    unsigned total;
    pre[w] = mesh_block_exclusive(__popc(o.first), &total, wsum);
    if (sdfk_tx() == 0) blk[sdfk_bx()] = total;
    int id = -1, cnt = 0;
    for (unsigned first = o.first; first; first &= first - 1u) {
        const int b = __builtin_ctz(first);
        const int child = label[p0 + b];
        if (child < 0 || child >= K) {
            atomicOr(err, TOPO_ERR_ID);
            continue;
        }
        if (child != id) {
            if (id >= 0) atomicAdd(supported + id, (unsigned long long)cnt);
            id = child;
            cnt = 0;
        }
        cnt += layer_stretch(o, b);
    }
    // what is left in the registers: one add per wave when every lane that has something has the same child
    const unsigned long long have = __ballot(id >= 0);
    if (!have) return;
    const int ref = __shfl(id, __builtin_ctzll(have), 64);
    if (__ballot(id >= 0 && id != ref)) {
        if (id >= 0) atomicAdd(supported + id, (unsigned long long)cnt);
        return;
    }
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if ((sdfk_tx() & 63) == 0) atomicAdd(supported + ref, (unsigned long long)cnt);
}

// links, emit: candidate `at` of the word order = (child << 32 | parent, length)
__global__ __launch_bounds__(SDFK_TOPO_THREADS) void sdfk_layer_emit_kernel(const unsigned* __restrict__ rb, const int* __restrict__ label,
                                                                            MeshGeom g, const unsigned long long* __restrict__ blk,
                                                                            const unsigned* __restrict__ pre, long long M,
                                                                            long long* __restrict__ key, int* __restrict__ length) {
    const long long w = (long long)sdfk_bx() * SDFK_TOPO_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    const LayerOverlap o = layer_overlap(rb, g, p0, rb[w]);
    long long at = (long long)blk[sdfk_bx()] + pre[w];
    for (unsigned first = o.first; first; first &= first - 1u, ++at) {
        const int b = __builtin_ctz(first);
        const long long p = p0 + b, q = p - g.s[0];             // (q >= 0: its bit came out of the bit string)
        if (at >= M || q < 0) continue;
        key[at] = ((long long)label[p] << 32) | (long long)(unsigned)label[q];
        length[at] = layer_stretch(o, b);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// The scratch is sdfk_label_scratch's, nothing added: the link pass keeps its per-tile counts in the mesh state's second
// tile array and its per-word prefixes in the prefix region the labelling leaves unused (1/8 B per point). The tag's fourth
// word holds the candidate count + 1 of the bits in the scratch (0: not counted yet).
static int layer_grid(int64_t n0, int64_t n1, int64_t n2, int* D, int64_t* dims, MeshGeom* g, const char* who) {
    if (n2 < 2) return fail(-1, std::string(who) + ": a stack has three axes (layers, u, v) of at least 2 points each");
    return topo_geom(n0, n1, n2, D, dims, g, who);
}

static int layer_label(const MeshSrc* src, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2, int64_t n2,
                       float level, int connectivity, int32_t* d_labels, int64_t* count, void* d_scratch, float* pass_ms,
                       hipStream_t stream, const char* who) {
    int D;
    int64_t dims[3];
    MeshGeom g;
    TopoScratch sc;
    int rc = layer_grid(n0, n1, n2, &D, dims, &g, who);
    if (rc) return rc;
    TopoEvents ev;
    if (src) {
        rc = ev.start(pass_ms);
        if (rc || (rc = ev.mark(stream))) return rc;
        if ((rc = topo_source(*src, ax0, n0, ax1, n1, ax2, n2, level, d_scratch, stream, who, &D, dims, &g, &sc))) return rc;
    } else {
        if (!d_scratch || ((uintptr_t)d_scratch & 255)) return fail(-1, std::string(who) + ": the scratch must be 256-byte aligned");
        topo_layout(D, dims, g.n, &sc, d_scratch);
        long long tag[3];
        if ((rc = topo_tag(sc, g, tag, who))) return rc;
        rc = ev.start(pass_ms);
        if (rc || (rc = ev.mark(stream))) return rc;
    }
    return topo_label(D, g, sc, connectivity, SDFK_REGION_INSIDE, d_labels, count, ev, pass_ms, stream, who, layer_launch_merge,
                      TOPO_TAG_LAYERED);
}

extern "C" int sdfk_field_layer_label(const float* d_field, const float* heights, int64_t layers, const float* u, int64_t nu,
                                      const float* v, int64_t nv, float level, int connectivity, int32_t* d_labels, int64_t* count,
                                      void* d_scratch, float* pass_ms, void* stream_) {
    const MeshSrc src{d_field, nullptr, 0};
    return layer_label(&src, heights, layers, u, nu, v, nv, level, connectivity, d_labels, count, d_scratch, pass_ms, (hipStream_t)stream_,
                       "sdfk_field_layer_label");
}

extern "C" int sdfk_eval_grid_layer_label(sdfk_program* p, const float* heights, int64_t layers, const float* u, int64_t nu,
                                          const float* v, int64_t nv, float level, int connectivity, int32_t* d_labels, int64_t* count,
                                          void* d_scratch, float* pass_ms, void* stream_, int mode) {
    const char* who = "sdfk_eval_grid_layer_label";
    if (!p) return fail(-1, std::string(who) + ": null program");
    const MeshSrc src{nullptr, p, mode};
    return layer_label(&src, heights, layers, u, nu, v, nv, level, connectivity, d_labels, count, d_scratch, pass_ms, (hipStream_t)stream_,
                       who);
}

extern "C" int sdfk_layer_label_bits(int64_t layers, int64_t nu, int64_t nv, int connectivity, int32_t* d_labels, int64_t* count,
                                     void* d_scratch, float* pass_ms, void* stream_) {
    return layer_label(nullptr, nullptr, layers, nullptr, nu, nullptr, nv, 0.0f, connectivity, d_labels, count, d_scratch, pass_ms,
                       (hipStream_t)stream_, "sdfk_layer_label_bits");
}

extern "C" int sdfk_layer_label_finish(int64_t layers, int64_t nu, int64_t nv, int64_t count, const int32_t* d_labels, int64_t* first,
                                       int64_t* sizes, int32_t* lower, int32_t* upper, int32_t* border, void* d_scratch,
                                       void* stream_) {
    const char* who = "sdfk_layer_label_finish";
    if (nv < 2) return fail(-1, std::string(who) + ": a stack has three axes (layers, u, v) of at least 2 points each");
    return topo_finish(layers, nu, nv, count, d_labels, first, sizes, lower, upper, border, d_scratch, stream_, true, who);
}

// the scratch of a layer labelling of `count` components on that grid -> sc, g, and the tag's four words
static int layer_scratch(int64_t layers, int64_t nu, int64_t nv, int64_t count, const void* d_labels, void* d_scratch, MeshGeom* g,
                         TopoScratch* sc, long long* tag, const char* who) {
    if (!d_scratch || ((uintptr_t)d_scratch & 255)) return fail(-1, std::string(who) + ": the scratch must be 256-byte aligned");
    if (!d_labels || count < 0) return fail(-1, std::string(who) + ": bad arguments");
    int D;
    int64_t dims[3];
    const int rc = layer_grid(layers, nu, nv, &D, dims, g, who);
    if (rc) return rc;
    topo_layout(D, dims, g->n, sc, d_scratch);
    HIPCHK(hipMemcpy(tag, sc->tag, 4 * sizeof(long long), hipMemcpyDeviceToHost));
    if (tag[0] != g->n || tag[1] != TOPO_TAG_LAYERED || tag[2] != count)
        return fail(-1, std::string(who) + ": the scratch does not hold a layer labelling of that grid and size");
    return 0;
}

extern "C" int sdfk_layer_links(int64_t layers, int64_t nu, int64_t nv, int64_t count, const int32_t* d_labels, int64_t* candidates,
                                int64_t* supported, void* d_scratch, void* stream_) {
    const char* who = "sdfk_layer_links";
    if (!candidates || (count > 0 && !supported)) return fail(-1, std::string(who) + ": bad arguments");
    hipStream_t stream = (hipStream_t)stream_;
    MeshGeom g;
    TopoScratch sc;
    long long tag[4];
    const int rc = layer_scratch(layers, nu, nv, count, d_labels, d_scratch, &g, &sc, tag, who);
    if (rc) return rc;
    *candidates = 0;
    const long long K = count;
    const unsigned tiles = (unsigned)sc.m.tiles;
    Scratch own;
    if (own.get(nullptr, mesh_align((size_t)std::max<long long>(K, 1) * 8)))
        return fail(-5, std::string(who) + ": out of device memory (the supported counts)");
    unsigned long long* d_supported = static_cast<unsigned long long*>(own.p);
    HIPCHK(hipMemsetAsync(d_supported, 0, (size_t)std::max<long long>(K, 1) * 8, stream));
    HIPCHK(hipMemsetAsync(sc.err, 0, sizeof(unsigned), stream));
    hipLaunchKernelGGL(sdfk_layer_count_kernel, dim3(tiles), dim3(SDFK_TOPO_THREADS), 0, stream, sc.rb, d_labels, g, K, sc.m.tblk, sc.m.tpre,
                       d_supported, sc.err);
    hipLaunchKernelGGL(sdfk_select_scan_kernel, dim3(1), dim3(1024), 0, stream, sc.m.tblk, (long long)tiles);
    hipError_t e = hipGetLastError();
    unsigned long long M = 0;
    unsigned err = 0;
    static_assert(sizeof(int64_t) == sizeof(unsigned long long), "counts are copied as they are");
    if (e == hipSuccess) e = hipMemcpyAsync(&M, sc.m.tblk + tiles, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&err, sc.err, sizeof(err), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && K) e = hipMemcpyAsync(supported, d_supported, (size_t)K * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    if (err) return fail(-7, std::string(who) + ": the array holds labels that are no ids below " + std::to_string(K));
    const long long counted = (long long)M + 1;
    HIPCHK(hipMemcpy(sc.tag + 3, &counted, sizeof(counted), hipMemcpyHostToDevice));
    *candidates = (int64_t)M;
    return 0;
}

extern "C" int sdfk_layer_links_finish(int64_t layers, int64_t nu, int64_t nv, int64_t count, const int32_t* d_labels,
                                       int64_t candidates, int64_t* keys, int32_t* lengths, void* d_scratch, void* stream_) {
    const char* who = "sdfk_layer_links_finish";
    if (candidates < 0 || (candidates > 0 && (!keys || !lengths))) return fail(-1, std::string(who) + ": bad arguments");
    hipStream_t stream = (hipStream_t)stream_;
    MeshGeom g;
    TopoScratch sc;
    long long tag[4];
    const int rc = layer_scratch(layers, nu, nv, count, d_labels, d_scratch, &g, &sc, tag, who);
    if (rc) return rc;
    if (tag[3] != candidates + 1) return fail(-1, std::string(who) + ": the scratch does not hold a link count of that size");
    if (candidates == 0) return 0;
    const long long M = candidates;
    const size_t b8 = mesh_align((size_t)M * 8), b4 = mesh_align((size_t)M * 4);
    Scratch own;
    if (own.get(nullptr, b8 + b4)) return fail(-5, std::string(who) + ": out of device memory (the candidates)");
    long long* d_key = static_cast<long long*>(own.p);
    int* d_len = reinterpret_cast<int*>(static_cast<char*>(own.p) + b8);
    hipLaunchKernelGGL(sdfk_layer_emit_kernel, dim3((unsigned)sc.m.tiles), dim3(SDFK_TOPO_THREADS), 0, stream, sc.rb, d_labels, g, sc.m.tblk,
                       sc.m.tpre, M, d_key, d_len);
    hipError_t e = hipGetLastError();
    static_assert(sizeof(int64_t) == sizeof(long long), "keys are copied as they are");
    if (e == hipSuccess) e = hipMemcpyAsync(keys, d_key, (size_t)M * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lengths, d_len, (size_t)M * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    return 0;
}
