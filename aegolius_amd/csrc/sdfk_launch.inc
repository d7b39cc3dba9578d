// Launch path: tile and row-block geometry, the candidate lists of chain-mode programs, and the evaluation runner.
// Included by sdfk.hip after sdfk_jit.inc.
// tile geometry of the brick-culling kernel: SDFK_TWAVES waves x SDFK_WBRICKS bricks of 128 points per
// workgroup (overridable through the environment for experiments)
static int tile_waves() {
    static int v = [] { const char* e = getenv("SDFK_TWAVES"); int t = e ? atoi(e) : 4; return (t >= 1 && t <= 16) ? t : 4; }();
    const int o = g_twaves_override.load();
    return o ? o : v;
}
static int tile_wbricks() {
    static int v = [] {
        const char* e = getenv("SDFK_WBRICKS");
        int t = e ? atoi(e) : 4;
        if (t < 1 || t > 32) t = 4;
        return t;
    }();
    return v;
}
static int tile_points() { return tile_waves() * tile_wbricks() * 128; }
// bricks per wave of the row-block kernel: 2 — except for big trees (> 150 instructions, e.g. the 50-primitive 2-D
// union), whose whole-tree probe is better shared by 16 bricks per workgroup than by 8 (measured -11 %)
// waves per workgroup of the row-block kernel: 4. (Round 2 measured 2 best, when ONE lane per brick probed the whole tree and
// a bigger workgroup only made more waves wait for it. Since the probe runs on all lanes — round 3 — the workgroup's serial
// steps, centres and fold on the first wave, are shared by more bricks: round 4, one box, 2 -> 4 waves: north-star tree
// 2.944 -> 2.913 ms, 20-primitive tree 3.356 -> 3.186 at 1025^3 and 25.4 -> 24.9 at 2049^3, 50-member flat union 0.847 ->
// 0.833, 513^3 1-2 %; 3, 6 and 8 waves are slower everywhere: profiles/r04_rwaves_sweep.txt.)
static int rows_waves(const sdfk_program*) {
    if (const int o = g_rwaves_override.load()) return o;
    return 4;
}
static int rows_wbricks(const sdfk_program* p);
// Programs that are not chains and hold more than SDFK_BIG_PROGRAM instructions (300) are built with two LLVM passes off
// (big_build_options): bit 16 of the geometry word, which selects the compiler options of a build and is part of its key
static long long big_program_limit() {
    static const long long v = [] {
        const char* e = getenv("SDFK_BIG_PROGRAM");
        const long long t = e ? atoll(e) : 300;
        return t > 0 ? t : 300;
    }();
    return v;
}
static int rows_geo(const sdfk_program* p) {
    const bool big = p && !p->chain_mode && (long long)(p->code.size() / 2) > big_program_limit();
    return rows_wbricks(p) | (rows_waves(p) << 4) | (big ? 1 << 16 : 0);
}
static int rows_wbricks(const sdfk_program* p) {
    static int forced = [] { const char* e = getenv("SDFK_RWBRICKS"); int t = e ? atoi(e) : 0; return (t >= 1 && t <= 16) ? t : 0; }();
    if (const int o = g_rwbricks_override.load()) return o;
    if (forced) return forced;
    // chain mode (measured, 513^3 sphere unions and the 50-child flat union): every brick of a wave costs a fold and an
    // evaluation pass one after the other, and the leaf values take 6 bytes of LDS per child and brick — few bricks per
    // wave win: 1000 spheres 21.9 / 11.4 / 5.5 ms with 4 / 2 / 1, the flat union 1.08 / 0.99 / 1.03 ms
    if (p && p->chain_mode) return p->chain_members <= 64 ? 2 : 1;
    // (rounds 2-3 gave programs beyond 150 instructions 4 bricks per wave; with skip bits for every site — SDFK_MASK_SITES —
    //  2 win at every size: 70 / 100 / 150 / 200 primitives at 513^3 1.40 / 1.87 / 2.79 / 3.51 ms against 1.55 / 2.34 / 3.18 /
    //  4.00, profiles/r04_bigtree_wbricks.txt)
    return 2;
}
struct RowGeom {           // mirrors sdfk_rowgeom of the generated source
    unsigned L, nchunk, nbricks;
    long long R;
    long long row0;
    int yrows;
    // row blocks never straddle a PLANE of the grid (rows of one x): the slab's rows are the rest of a first plane
    // (seg0 rows, nb0 blocks), then planes of prow rows (bpp blocks each; the last block of a plane may be partial)
    unsigned prow, seg0, nb0, bpp;
    unsigned inv_nchunk, inv_bpp;                              // floor(2^32 / nchunk), floor(2^32 / bpp) (sdfk_udiv)
};
// can the row-block kernel take n points in rows of row_len? (brick ids are 32-bit)
// plane_rows: rows per grid plane (0 / >= R: one plane — blocks of 16 consecutive rows throughout);
// plane_phase: index within its plane of the first row. Both are layout hints like row_len: they only decide which
// 16 rows form a block (a block of rows from two planes has a bounding sphere as wide as the grid and culls nothing).
static bool rows_geometry(long long n, long long row_len, RowGeom* g, long long plane_rows = 0, long long plane_phase = 0,
                          bool planes_on = false) {
    if (row_len < 32 || row_len > 0x7fffffffLL || n <= 0 || n % row_len != 0) return false;
    const long long R = n / row_len, brows = 16;
    // windows of 32 points aligned in the flat array: one more than ceil(L / 32) can overlap a row
    const long long nchunk = (row_len % 32 == 0) ? row_len / 32 : (row_len + 62) / 32;
    long long prow = plane_rows, seg0 = 0;
    // Measured on 513^3 / 1025^3 (tools/rows_ab.py `noplanes:`): the partial block that ends every plane of 2^k + 1 rows
    // costs as much as the one straddling block it replaces saves (513^3: 0.413 vs 0.401 ms, 1025^3 equal) — so the hint
    // is honoured only on request (SDFK_PLANE_BLOCKS=1); the default is blocks of 16 consecutive rows throughout.
    static const bool plane_blocks = [] { const char* e = getenv("SDFK_PLANE_BLOCKS"); return e && e[0] == '1'; }();
    if (!(plane_blocks || planes_on) || prow <= 0 || prow >= R || prow > 0x7fffffffLL) {
        prow = R > 0x7fffffffLL ? 0 : R;                       // one plane
        if (prow == 0) return false;
    } else if (plane_phase > 0) {
        seg0 = std::min(R, (prow - plane_phase % prow) % prow);
    }
    const long long nb0 = (seg0 + brows - 1) / brows, bpp = (prow + brows - 1) / brows;
    const long long planes = (R - seg0 + prow - 1) / prow;
    const long long nb = nchunk * (nb0 + planes * bpp);
    if (nb > 0x7fffffffLL - 1024) return false;
    g->L = (unsigned)row_len;
    g->nchunk = (unsigned)nchunk;
    g->nbricks = (unsigned)nb;
    g->R = R;
    g->row0 = 0;
    g->yrows = 0;
    g->prow = (unsigned)prow;
    g->seg0 = (unsigned)seg0;
    g->nb0 = (unsigned)nb0;
    g->bpp = (unsigned)bpp;
    g->inv_nchunk = (unsigned)std::min<unsigned long long>(0xffffffffull, (1ull << 32) / (unsigned long long)nchunk);
    g->inv_bpp = (unsigned)std::min<unsigned long long>(0xffffffffull, (1ull << 32) / (unsigned long long)bpp);
    return true;
}
static int tile_threads() { return 64 * tile_waves(); }
static inline unsigned blocks_for(long long n, int vec) {
    return (unsigned)((n + (long long)SDFK_BLOCK * vec - 1) / ((long long)SDFK_BLOCK * vec));
}

// test aid: statistics of the candidate lists of the last chain-mode launch (sdfk_debug_cells_stats)
static std::atomic<bool> g_cells_stats_on{false};
static std::mutex g_cells_stats_mu;
static long long g_cells_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
extern "C" void sdfk_debug_cells_stats(int enable, long long* out8) {
    g_cells_stats_on.store(enable != 0);
    if (out8) {
        std::lock_guard<std::mutex> lk(g_cells_stats_mu);
        for (int i = 0; i < 8; ++i) out8[i] = g_cells_stats[i];
        for (int i = 0; i < 8; ++i) g_cells_stats[i] = 0;
    }
}
// ---- candidate lists of chain-mode programs (sdfk_codegen.cpp: sdfk_cells / sdfk_cellpass / sdfk_spec_cells) ------------------
struct CellLevelH {           // mirrors sdfk_celllevel
    unsigned lx, ly, lz, ncx, ncy, ncz, xoff, pad;
};
struct CellsArg {             // mirrors sdfk_cells
    CellLevelH lv;
    const void *sph, *span, *cand;
    unsigned enabled, ncells;
};
struct CellPassArg {          // mirrors sdfk_cellpass
    CellLevelH lv, parent;
    void *sph, *span;
    const void *psph, *pspan;
    void* cand;
    unsigned* head;
    unsigned base, shard_cap;
    unsigned ncells, pad0;
    float inflate, pad;
};
static bool parse3(const char* e, unsigned* v) {
    int a = 0, b = 0, c = 0;
    if (!e || sscanf(e, "%d,%d,%d", &a, &b, &c) != 3 || a < 0 || b < 0 || c < 0 || a > 12 || b > 12 || c > 12) return false;
    v[0] = (unsigned)a; v[1] = (unsigned)b; v[2] = (unsigned)c;
    return true;
}
static CellLevelH cell_level(const RowGeom& rg, const unsigned l[3]) {
    CellLevelH lv{};
    lv.lx = l[0]; lv.ly = l[1]; lv.lz = l[2];
    const long long planes = rg.prow ? ((rg.R - rg.seg0) + rg.prow - 1) / rg.prow : 0;
    lv.xoff = rg.seg0 > 0 ? (1u << lv.lx) : 0u;
    lv.ncx = planes > 0 ? (unsigned)(((long long)lv.xoff + planes - 1) >> lv.lx) + 1u : 1u;
    lv.ncy = ((std::max(rg.bpp, rg.nb0) - 1u) >> lv.ly) + 1u;
    lv.ncz = ((rg.nchunk - 1u) >> lv.lz) + 1u;
    return lv;
}
// Lists for this launch: sizes the levels, (re)allocates the stream's scratch, enqueues the pre-pass (coarse level, then
// fine) on `stream` and fills what the row-block kernel is handed. cells_fn: sdfk_spec_cells / sdfk_spec_cellsg of the
// module, `src`: its first kernel arguments after PRM / TAB (array: co, stride; grid: the SrcGrid), n_src of them.
static int prepare_cells(sdfk_program* p, DevState* d, hipFunction_t cells_fn, const RowGeom& rg, void** src, int n_src,
                         const float* prm, const float* tab, hipStream_t stream, CellsArg* out) {
    memset(out, 0, sizeof *out);
    static const int min_members = [] { const char* e = getenv("SDFK_CELLS_MIN"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 17; }();
    static const bool off = [] { const char* e = getenv("SDFK_CELLS"); return e && e[0] == '0'; }();
    if (!cells_fn || off || p->chain_members < min_members) return 0;
    const bool is3d = rg.prow < (unsigned long long)rg.R;
    unsigned lf[3] = {is3d ? 3u : 0u, is3d ? 1u : 2u, is3d ? 0u : 1u};            // 8 planes x 32 rows x 32 points | 64 rows x 64 points
    unsigned lc[3] = {lf[0] + (is3d ? 2u : 0u), lf[1] + 2u, lf[2] + 2u};          // 4 x 4 x 4 (4 x 4) fine cells
    static const char* e_fine = getenv("SDFK_CELL_FINE");
    static const char* e_coarse = getenv("SDFK_CELL_COARSE");
    (void)parse3(e_fine, lf);
    bool coarse = p->chain_members >= 128;
    if (e_coarse) coarse = parse3(e_coarse, lc);
    if (coarse && (lc[0] < lf[0] || lc[1] < lf[1] || lc[2] < lf[2])) coarse = false;
    const CellLevelH fine = cell_level(rg, lf);
    const CellLevelH crs = coarse ? cell_level(rg, lc) : CellLevelH{};
    const unsigned long long nf = (unsigned long long)fine.ncx * fine.ncy * fine.ncz;
    const unsigned long long nc = coarse ? (unsigned long long)crs.ncx * crs.ncy * crs.ncz : 0ull;
    if (nf == 0 || nf > 0x3fffffffull || nc > 0x3fffffffull) return 0;
    // pool: room for 48 entries per fine cell and 1024 per coarse cell (measured lists: a handful / a few hundred); a cell
    // that finds the pool full makes its bricks probe every member — slower, never wrong
    // Pool of list entries, per level 256 shards with an allocation head each (sdfk_cells_kernel). The coarse level can
    // never run out — a shard holds every member for each of its cells —; the fine level gets 256 entries per cell plus
    // slack (measured lists: a handful to a few dozen entries, a few hundred in scenes where thousands of members overlap).
    const unsigned long long members = (unsigned long long)p->chain_members, shards = 256;
    unsigned long long cshard = ((nc + shards - 1) / shards) * members;
    // (a fine shard serves ceil(cells / 256) cells: every member for each of them, or the budget — but never less than one
    //  whole list)
    unsigned long long fshard = std::max(members, std::min(((nf + shards - 1) / shards) * members, (256ull * nf + (16ull << 20) + shards - 1) / shards));
    if (const char* e = getenv("SDFK_CELLS_POOL")) {             // (tests: a pool too small for the lists)
        const long long v = atoll(e);
        if (v > 0) fshard = std::min<unsigned long long>(fshard, (unsigned long long)v);
    }
    if (shards * (cshard + fshard) > 0x3fffffffull) return 0;   // (no lists: still correct)
    const unsigned long long cap = shards * (cshard + fshard);
    const size_t o_fsph = 0, o_fspan = o_fsph + 16 * nf, o_csph = o_fspan + 8 * nf, o_cspan = o_csph + 16 * nc,
                 o_head = (o_cspan + 8 * nc + 63) & ~(size_t)63, o_pool = o_head + 2 * 64 * shards, total = o_pool + 4 * cap + 64;
    CellScratch* cs;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        cs = &d->cells[stream];
    }
    if (cs->bytes < total) {
        if (cs->buf) {
            HIPCHK(hipStreamSynchronize(stream));              // (the stream's earlier launches read the old buffer)
            (void)hipFree(cs->buf);
            cs->buf = nullptr;
            cs->bytes = 0;
        }
        if (hipMalloc(&cs->buf, total + total / 4) != hipSuccess) { (void)hipGetLastError(); return 0; }   // (no lists: still correct)
        cs->bytes = total + total / 4;
    }
    char* b = cs->buf;
    HIPCHK(hipMemsetAsync(b + o_head, 0, 2 * 64 * shards, stream));
    CellPassArg cp{};
    cp.cand = b + o_pool;
    if (coarse) {
        // a coarse cell answers for 1.3 x its circumsphere: room for the circumspheres of the fine cells inside it
        cp.lv = crs; cp.parent = CellLevelH{}; cp.sph = b + o_csph; cp.span = b + o_cspan; cp.psph = nullptr; cp.pspan = nullptr;
        cp.ncells = (unsigned)nc; cp.inflate = 1.3f;
        cp.head = reinterpret_cast<unsigned*>(b + o_head);
        cp.base = 0u; cp.shard_cap = (unsigned)cshard;
        std::vector<void*> args = {(void*)&prm, (void*)&tab};
        for (int i = 0; i < n_src; ++i) args.push_back(src[i]);
        RowGeom g2 = rg;
        args.push_back(&g2);
        args.push_back(&cp);
        HIPCHK(hipModuleLaunchKernel(cells_fn, (unsigned)((nc + 3) / 4), 1, 1, 256, 1, 1, 0, stream, args.data(), nullptr));
    }
    cp.lv = fine; cp.parent = coarse ? crs : CellLevelH{}; cp.sph = b + o_fsph; cp.span = b + o_fspan;
    cp.psph = coarse ? b + o_csph : nullptr; cp.pspan = coarse ? b + o_cspan : nullptr;
    cp.ncells = (unsigned)nf; cp.inflate = 1.0f;
    cp.head = reinterpret_cast<unsigned*>(b + o_head + 64 * shards);
    cp.base = (unsigned)(shards * cshard); cp.shard_cap = (unsigned)fshard;
    {
        std::vector<void*> args = {(void*)&prm, (void*)&tab};
        for (int i = 0; i < n_src; ++i) args.push_back(src[i]);
        RowGeom g2 = rg;
        args.push_back(&g2);
        args.push_back(&cp);
        HIPCHK(hipModuleLaunchKernel(cells_fn, (unsigned)((nf + 3) / 4), 1, 1, 256, 1, 1, 0, stream, args.data(), nullptr));
    }
    static const bool trace = [] { const char* e = getenv("SDFK_CELLS_TRACE"); return e && e[0] == '1'; }();
    if (trace || g_cells_stats_on.load()) {                      // (debug: synchronises and reads the lists' statistics back)
        HIPCHK(hipStreamSynchronize(stream));
        std::vector<uint2> sp(nf);
        unsigned head = 0;
        HIPCHK(hipMemcpy(sp.data(), b + o_fspan, 8 * nf, hipMemcpyDeviceToHost));
        {
            std::vector<unsigned> heads(2 * 16 * shards);
            HIPCHK(hipMemcpy(heads.data(), b + o_head, 2 * 64 * shards, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < heads.size(); i += 16) head += heads[i];
        }
        unsigned long long sum = 0, all = 0, empty = 0, mx = 0;
        for (const uint2& x : sp) {
            if (x.y == 0xffffffffu) ++all;
            else { sum += x.y; mx = std::max<unsigned long long>(mx, x.y); if (x.y == 0) ++empty; }
        }
        {
            std::lock_guard<std::mutex> lk(g_cells_stats_mu);
            g_cells_stats[0] = (long long)nf; g_cells_stats[1] = (long long)nc; g_cells_stats[2] = (long long)head;
            g_cells_stats[3] = (long long)cap; g_cells_stats[4] = (long long)sum; g_cells_stats[5] = (long long)mx;
            g_cells_stats[6] = (long long)all; g_cells_stats[7] = (long long)empty;
        }
        if (trace) fprintf(stderr, "[sdfk cells] %d members: fine %ux%ux%u = %llu cells (2^%u planes x 2^%u blocks x 2^%u windows), coarse %llu; pool %u of %llu entries; "
                "fine lists: mean %.1f max %llu, %llu without a list, %llu empty\n", p->chain_members, fine.ncx, fine.ncy, fine.ncz, nf, fine.lx, fine.ly, fine.lz, nc,
                head, cap, (double)sum / (double)std::max<unsigned long long>(1, nf - all - empty), mx, all, empty);
    }
    out->lv = fine;
    out->sph = b + o_fsph;
    out->span = b + o_fspan;
    out->cand = b + o_pool;
    out->enabled = 1u;
    out->ncells = (unsigned)nf;
    return 0;
}

// ---- the launch context every kernel of a program starts from ------------------------------------------------------
// current device, the program resident on it (ensure_resident), and what each launch is handed from there
struct LaunchCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    DevState* d = nullptr;
    const float* prm = nullptr;
    const float* tab = nullptr;
    int n_instr = 0, result_reg = 0;
};
static int launch_ctx(sdfk_program* p, void* stream, LaunchCtx* c) {
    c->stream = (hipStream_t)stream;
    HIPCHK(hipGetDevice(&c->device));
    const int rc = ensure_resident(p, c->device, c->stream, &c->d);
    if (rc) return rc;
    c->prm = c->d->d_params;
    c->tab = c->d->d_tables;
    c->n_instr = (int)(p->code.size() / 2);
    c->result_reg = p->result_reg;
    return 0;
}
// Small or full register file: the kernels that interpret a program exist in two instantiations, and a launch takes the
// small one when the program fits it. GO(NC, NV) is the launch; NC_FULL / NV_FULL the full file of that kernel
// (SDFK_NC / SDFK_NV, or SDFK_DUAL_NC / SDFK_DUAL_NV for the dual, adjoint and enclosure kernels).
#define SDFK_REGFILE(p, NC_FULL, NV_FULL, GO)                \
    do {                                                     \
        if ((p)->interp_small) GO(SDFK_NC_SMALL, SDFK_NV_SMALL); \
        else GO(NC_FULL, NV_FULL);                           \
    } while (0)

// ---- which kernel serves a call ------------------------------------------------------------------------------------
// The module of `flavour` (build variants `variant`: get_module) for a call in the resolved `mode`, or *sk == nullptr:
// the interpreter kernel serves the call — mode INTERPRET; AUTO while hiprtc is still building the flavour (background
// thread, SDFK_ASYNC_JIT=0 turns that off: the same device functions, the same bits, later calls switch over);
// or a build that failed where the caller lets the call fall back (`may_fall_back`). Every other mode waits for the build.
// what: "kernel", "ray kernel", ... of the error text; warn: one line on stderr, once per process, when a call falls back.
static int pick_kernel(sdfk_program* p, int device, int flavour, int variant, int mode, bool may_fall_back, const char* what,
                       bool warn, std::shared_ptr<SpecModule>* sk) {
    sk->reset();
    if (mode != SDFK_MODE_INTERPRET) {
        static const bool async_jit = [] { const char* e = getenv("SDFK_ASYNC_JIT"); return !(e && e[0] == '0'); }();
        const bool wait = mode != SDFK_MODE_AUTO || !p->interp_ok || !async_jit;
        std::string err;
        *sk = get_module(p, device, flavour, wait, &err, variant);
        if (*sk && (*sk)->failed) {
            if (!may_fall_back || !p->interp_ok) return fail(-3, std::string("specialised ") + what + " unavailable: " + err);
            static bool warned = false;
            if (warn && !warned) {
                fprintf(stderr, "[sdfk] hiprtc specialisation failed, using the interpreter kernel: %s\n", err.c_str());
                warned = true;
            }
            sk->reset();
        }
    }
    if (!*sk && !p->interp_ok)
        return fail(-4, "program needs more registers than the interpreter kernel has (use the specialised mode)");
    return 0;
}

// ---- one evaluation: the request, the plan, the two launches -------------------------------------------------------
struct EvalPlan;
// What an evaluation is asked to do. Callers fill in what they use; every other field keeps its default.
struct EvalCall {
    sdfk_program* p = nullptr;
    const SrcArray* arr = nullptr;        // the coordinates: a (3, n) array ...
    const SrcGrid* grid = nullptr;        // ... or per-axis grid tables (exactly one of the two)
    long long n = 0;
    float* d_out = nullptr;
    void* stream = nullptr;
    int mode = SDFK_MODE_AUTO;
    bool vec_ok = false;                  // rows and output are 16-byte aligned: 4-wide body, line bricks
    // layout hints of an array (grids know theirs): its points are grid rows of row_len points; `flat`: rows of a flat
    // grid (z = 0, rows along y); plane_rows rows per grid plane, the first row the plane_phase-th of its plane
    long long row_len = 0;
    bool flat = false;
    long long plane_rows = 0, plane_phase = 0;
    const float* aux = nullptr;           // auxiliary per-point fields of a staged program, rows of aux_stride
    long long aux_stride = 0;
    unsigned* d_flags = nullptr;          // fused selection: flag words (key <= thr_key) instead of the field
    unsigned thr_key = 0;
    bool xy = false;                      // the array has two rows, z = 0 by contract
    const EvalPlan* plan = nullptr;       // the caller has planned this very request (it laid its flag words out from it)
};
// the request of a grid / an array evaluation in its common fields: `n` points (a grid's from g->start on)
static EvalCall grid_call(sdfk_program* p, const SrcGrid* g, long long n, float* d_out, void* stream, int mode, bool vec_ok) {
    EvalCall c;
    c.p = p;
    c.grid = g;
    c.n = n;
    c.d_out = d_out;
    c.stream = stream;
    c.mode = mode;
    c.vec_ok = vec_ok;
    return c;
}
static EvalCall array_call(sdfk_program* p, const SrcArray* a, long long n, float* d_out, void* stream, int mode, bool vec_ok) {
    EvalCall c = grid_call(p, nullptr, n, d_out, stream, mode, vec_ok);
    c.arr = a;
    return c;
}
// The env-derived inputs of the planner (read once per process) and the process-wide default mode.
// Build time bounds (programs that are not chains: those are table-driven and build in under a second whatever their
// size). hiprtc's time grows faster than the program — profiles/r04_build_time.txt, left-deep smooth-union chains on
// the build container's CPU: row blocks 1 / 4 / 8 / 21 / 102 s at 29 / 89 / 179 / 299 / 449 instructions with the full
// pipeline; beyond SDFK_BIG_PROGRAM (300) instructions builds run without CodeGenPrepare and VectorCombine
// (rtc_options): row blocks 21 / 30 / 49 / 85 s at 449 / 599 / 899 / 1199, line bricks 8 / 11 / 22 / 33 s, the plain
// kernel 4 / 6 / 12 / 25 s (on the GPU boxes' CPUs less than half of that). With skip bits for 512 sites a row-block
// kernel is 2-3 x a line-brick one on these programs, so both limits are the same now:
//   row blocks up to SDFK_ROWS_LIMIT instructions (1200), line bricks (or, for unaligned arrays, the plain kernel) up to
//   SDFK_SPECIALIZE_LIMIT (1200); beyond that AUTO stays on the interpreter kernel, which needs no compilation.
// A background build that is still running when the process leaves is killed (sdfk_jit_cancel).
// MODE_SPECIALIZED / NOCULL always build (the caller asked for the kernel and waits), with the same choice of flavour.
struct PlanEnv {
    int default_mode;
    long long spec_limit, rows_limit;
};
static PlanEnv plan_env() {
    static const auto limit = [](const char* name) {
        const char* e = getenv(name);
        const long long v = e ? atoll(e) : 1200;
        return v > 0 ? v : 1200;
    };
    static const long long spec_limit = limit("SDFK_SPECIALIZE_LIMIT"), rows_limit = limit("SDFK_ROWS_LIMIT");
    return {g_default_mode, spec_limit, rows_limit};
}
struct EvalPlan {
    int mode = SDFK_MODE_AUTO;            // resolved: never AUTO unless that is the default mode
    int flavour = SDFK_FL_PLAIN_ARRAY;    // the kernel family a specialised launch takes (INTERPRET: none is built)
    RowGeom rg = {};                      // of the row-block flavours
    int variant = 0;                      // build variants of get_module: bit 0 flag-writing, bit 1 two-row coordinates
    bool needs_specialised = false;       // flags or two-row coordinates: the interpreter kernel cannot serve this call
    bool rows() const {
        return flavour == SDFK_FL_ROWS_ARRAY || flavour == SDFK_FL_ROWS_GRID || flavour == SDFK_FL_ROWS2D_ARRAY ||
               flavour == SDFK_FL_ROWS2D_GRID;
    }
    bool tile() const { return flavour == SDFK_FL_TILE_ARRAY || flavour == SDFK_FL_TILE_GRID; }
};
// Which kernel does this call get? Host arithmetic only — no device, no HIP call: sdfk_debug_eval_plan shows it to tests.
// Expects c.p, c.n > 0 and one source.
static int plan_eval(const EvalCall& c, const PlanEnv& env, EvalPlan* out) {
    const sdfk_program* p = c.p;
    const bool flags = c.d_flags != nullptr;
    const long long n_instr = (long long)(p->code.size() / 2);
    EvalPlan pl;
    int mode = c.mode;
    if (mode == SDFK_MODE_AUTO) mode = env.default_mode;
    // flags instead of the field (fused selection): the specialised plain / row-block kernels only — the call waits for
    // their build instead of starting on the interpreter kernel
    if (flags && (mode == SDFK_MODE_AUTO || mode == SDFK_MODE_INTERPRET)) mode = SDFK_MODE_SPECIALIZED;
    // two-row coordinates (z = 0 by contract): builds of the plain and the flat row-block array kernels that never touch a
    // third row; the interpreter kernel has no such build, so these calls wait for the specialised kernel too
    if (c.xy) {
        if (!c.arr || p->n_aux > 0) return fail(-1, "two-row coordinates: array source, no auxiliary fields");
        if (mode == SDFK_MODE_AUTO || mode == SDFK_MODE_INTERPRET) mode = SDFK_MODE_SPECIALIZED;
    }
    pl.needs_specialised = flags || c.xy;
    pl.variant = (flags ? 1 : 0) | (c.xy ? 2 : 0);
    if (mode == SDFK_MODE_AUTO && n_instr > env.spec_limit && p->interp_ok && !p->chain_mode && !flags)
        mode = SDFK_MODE_INTERPRET;

    // Which flavour does this call launch? (row blocks > line bricks > plain; NOCULL and programs without sites: plain)
    const SrcGrid* grid = c.grid;
    pl.flavour = c.arr ? SDFK_FL_PLAIN_ARRAY : SDFK_FL_PLAIN_GRID;
    const long long grow = grid ? (grid->n2 > 1 ? (long long)grid->n2 : (long long)grid->n1) : 0;
    if (!p->sites.empty() && mode != SDFK_MODE_NOCULL && mode != SDFK_MODE_INTERPRET) {
        // (chain mode: row blocks of ONE plane each — the cells of its candidate lists are boxes of the grid)
        if (c.arr && rows_geometry(c.n, c.row_len, &pl.rg, (c.flat || flags) ? 0 : c.plane_rows, c.plane_phase, p->chain_mode))
            pl.flavour = (c.flat || c.xy) ? SDFK_FL_ROWS2D_ARRAY : SDFK_FL_ROWS_ARRAY;   // rows need no alignment beyond 4 bytes
        else if (c.arr && c.vec_ok && !p->chain_mode && !flags && !c.xy) pl.flavour = SDFK_FL_TILE_ARRAY;
        else if (grid && grid->start % grow == 0 &&
                 rows_geometry(c.n, grow, &pl.rg, (grid->n2 > 1 && !flags) ? (long long)grid->n1 : 0,    // (flags: the slot layout
                               grid->n2 > 1 ? (grid->start / grow) % (long long)grid->n1 : 0, p->chain_mode))   //  knows blocks of 16 rows)
            pl.flavour = grid->n2 > 1 ? SDFK_FL_ROWS_GRID : SDFK_FL_ROWS2D_GRID;
        else if (grid && c.vec_ok && !p->chain_mode && !flags) pl.flavour = SDFK_FL_TILE_GRID;
        // (too big for a row-block build within the budget: the line-brick kernel where the call allows it, else un-culled)
        if (!p->chain_mode && n_instr > env.rows_limit && pl.rows()) {
            const bool is_arr = c.arr != nullptr;
            if (c.vec_ok && !flags && !c.xy) pl.flavour = is_arr ? SDFK_FL_TILE_ARRAY : SDFK_FL_TILE_GRID;
            else if (!flags) pl.flavour = is_arr ? SDFK_FL_PLAIN_ARRAY : SDFK_FL_PLAIN_GRID;
        }
    }
    if (grid && pl.rows()) {
        // whole grid rows (x-slabs of a sharded evaluation always are); rows along the third axis, or along the second
        // one when the grid is flat (n2 == 1)
        pl.rg.row0 = grid->start / grow;
        pl.rg.yrows = grid->n2 > 1 ? 0 : 1;
    }
    pl.mode = mode;
    *out = pl;
    return 0;
}

static int launch_specialised(const EvalCall& c, const EvalPlan& pl, const LaunchCtx& x, const SpecModule& sk) {
    sdfk_program* p = c.p;
    const float *prm = x.prm, *tab = x.tab, *aux = c.aux, *co = c.arr ? c.arr->co : nullptr;
    long long n = c.n, aux_stride = c.aux_stride, stride = c.arr ? c.arr->stride : 0;
    float* d_out = c.d_out;
    unsigned* d_flags = c.d_flags;
    unsigned thr_key = c.thr_key;
    SrcGrid g = c.grid ? *c.grid : SrcGrid{};
    // every kernel's arguments: PRM, TAB, the source (array: co, stride; grid: the SrcGrid), then its own
    void* args[13] = {&prm, &tab, &co, &stride};
    if (c.grid) args[2] = &g;
    const int n_src = c.grid ? 1 : 2;
    auto go = [&](hipFunction_t fn, unsigned blocks, unsigned threads, std::initializer_list<void*> own) {
        std::copy(own.begin(), own.end(), args + 2 + n_src);
        return hipModuleLaunchKernel(fn, blocks, 1, 1, threads, 1, 1, 0, x.stream, args, nullptr);
    };
    if (pl.rows()) {
        RowGeom rg = pl.rg;
        const unsigned per_tile = (unsigned)(rows_waves(p) * rows_wbricks(p));
        const unsigned tiles = ((rg.nbricks + per_tile - 1) / per_tile + 127u) & ~127u;   // whole rounds of 8 XCDs x SDFK_XGROUP = 16 tiles (sdfk_codegen.cpp)
        // (chain-mode builds take one more argument, their candidate lists: prepare_cells; fn[1] = the pre-pass kernel)
        CellsArg cells{};
        if (p->chain_mode && sk.fn[1] != nullptr) {
            const int rc = prepare_cells(p, x.d, sk.fn[1], rg, args + 2, n_src, prm, tab, x.stream, &cells);
            if (rc) return rc;
        }
        HIPCHK(go(sk.fn[0], tiles, 64u * (unsigned)rows_waves(p), {&rg, &d_out, &d_flags, &thr_key, &cells}));
    } else if (pl.tile()) {
        // brick-culling tile kernel: handles the ragged end itself
        HIPCHK(go(sk.fn[0], (unsigned)((n + tile_points() - 1) / tile_points()), tile_threads(), {&n, &d_out}));
    } else {
        // plain: a 4-wide body (fn[0]) and a scalar tail (fn[1])
        long long n4 = c.vec_ok ? (n / 4) * 4 : 0, tail = n - n4, zero = 0;
        if (n4) HIPCHK(go(sk.fn[0], blocks_for(n4, 4), SDFK_BLOCK, {&zero, &n4, &d_out, &aux, &aux_stride, &d_flags, &thr_key}));
        if (tail) HIPCHK(go(sk.fn[1], blocks_for(tail, 1), SDFK_BLOCK, {&n4, &tail, &d_out, &aux, &aux_stride, &d_flags, &thr_key}));
    }
    return 0;
}

static int launch_interpreter(const EvalCall& c, const LaunchCtx& x) {
    const sdfk_program* p = c.p;
    const long long n4 = c.vec_ok ? (c.n / 4) * 4 : 0, tail = c.n - n4, zero = 0;   // a 4-wide body and a scalar tail
    auto launch = [&](auto src, int vec, long long off, long long cnt) {
        using SRC = decltype(src);
        const dim3 grid(blocks_for(cnt, vec)), block(SDFK_BLOCK);
#define SDFK_INTERP_GO4(NC, NV) hipLaunchKernelGGL((sdfk_interp_kernel<4, NC, NV, SRC>), grid, block, 0, x.stream, x.d->d_code, \
                                                   x.n_instr, x.prm, x.tab, src, off, cnt, c.d_out, x.result_reg, c.aux, c.aux_stride)
#define SDFK_INTERP_GO1(NC, NV) hipLaunchKernelGGL((sdfk_interp_kernel<1, NC, NV, SRC>), grid, block, 0, x.stream, x.d->d_code, \
                                                   x.n_instr, x.prm, x.tab, src, off, cnt, c.d_out, x.result_reg, c.aux, c.aux_stride)
        if (vec == 4) SDFK_REGFILE(p, SDFK_NC, SDFK_NV, SDFK_INTERP_GO4);
        else SDFK_REGFILE(p, SDFK_NC, SDFK_NV, SDFK_INTERP_GO1);
#undef SDFK_INTERP_GO4
#undef SDFK_INTERP_GO1
    };
    if (c.arr) {
        if (n4) launch(*c.arr, 4, zero, n4);
        if (tail) launch(*c.arr, 1, n4, tail);
    } else {
        if (n4) launch(*c.grid, 4, zero, n4);
        if (tail) launch(*c.grid, 1, n4, tail);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// The evaluation runner: plan (unless the caller has), make the program resident, pick the kernel, launch.
static int run(const EvalCall& c) {
    sdfk_program* p = c.p;
    if (!p) return fail(-1, "null program");
    if (c.n < 0) return fail(-1, "negative point count");
    if (p->n_aux > 0 && (!c.aux || c.aux_stride < c.n))
        return fail(-1, "this program reads auxiliary fields (staged evaluation): use sdfk_eval_device_aux / sdfk_eval_grid_aux");
    if (c.n == 0) return 0;
    EvalPlan own;
    int rc = c.plan ? 0 : plan_eval(c, plan_env(), &own);
    if (rc) return rc;
    const EvalPlan& pl = c.plan ? *c.plan : own;
    LaunchCtx x;
    rc = launch_ctx(p, c.stream, &x);
    if (rc) return rc;
    // a failed build: AUTO and NOCULL fall back to the interpreter kernel — unless the call has no interpreter form
    std::shared_ptr<SpecModule> sk;
    rc = pick_kernel(p, x.device, pl.flavour, pl.variant, pl.mode, pl.mode != SDFK_MODE_SPECIALIZED && !pl.needs_specialised,
                     "kernel", true, &sk);
    if (rc) return rc;
    return sk ? launch_specialised(c, pl, x, *sk) : launch_interpreter(c, x);
}
