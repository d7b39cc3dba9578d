/* sdfk.h — C-ABI of libsdfk.so, the MI355X (gfx950) SDF grid-evaluation engine.
 *
 * The reference (peterropac/Aegolius = SPOMSO, pure Python) has no FFI seam; its seam is the
 * Python object protocol `GenericGeometry.create(co) -> (N,)`
 * (reference Code/spomso/spomso/cores/geom.py:29-43). The Python layer in aegolius_amd/ keeps that
 * protocol and lowers the expression tree it records to the register-machine program consumed here.
 * Each entry point below names the reference interface whose work it replaces.
 *
 * Conventions: plain C types only; 0 = success, negative = error (text via sdfk_last_error(),
 * thread-local); the caller owns every host buffer for the duration of a call; the library owns
 * programs and the device memory it allocates; programs are immutable after creation and may be
 * shared between threads; "device pointers" are ordinary HIP device addresses (for example
 * torch.Tensor.data_ptr() of a ROCm tensor) and `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).
 */
#ifndef SDFK_H
#define SDFK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFK_ABI_VERSION 1

/* evaluation modes for sdfk_eval_device / sdfk_set_default_mode */
#define SDFK_MODE_AUTO 0        /* topology-specialised kernel (hiprtc): only the kernel flavour a call launches is built,
                                   in a background thread, and cached (per process and on disk); until it is ready calls
                                   are served by the interpreter kernel (bit-identical results; SDFK_ASYNC_JIT=0: wait
                                   instead). The background build runs in a CHILD PROCESS (aegolius_amd/sdfk_rtc_helper:
                                   hiprtc inside the caller deadlocks against a dlopen of any HIP library on another
                                   thread); without the helper the first call waits. Build time is bounded by program
                                   size (programs that run in chain mode — sdfk_program_set_cull — build in under a
                                   second whatever their size): row-block kernels up to SDFK_ROWS_LIMIT (env, default
                                   1200) instructions, line bricks / plain up to SDFK_SPECIALIZE_LIMIT (1200), beyond that
                                   the interpreter kernel serves the program; from SDFK_BIG_PROGRAM (300) instructions on
                                   a build runs without LLVM's CodeGenPrepare and VectorCombine passes (quadratic in a
                                   straight-line program; same FP semantics, same bits) */
#define SDFK_MODE_INTERPRET 1   /* generic register-machine interpreter kernel */
#define SDFK_MODE_SPECIALIZED 2 /* wait for the specialised kernel; fail instead of falling back if hiprtc fails */
#define SDFK_MODE_NOCULL 3      /* specialised kernel with brick culling switched off (A/B runs, tests); along rays: the
                                   plain ray kernel, without the per-wave survivor lists of long unions */

typedef struct sdfk_program sdfk_program;

int sdfk_abi_version(void);
/* number of visible HIP devices (0 when there is no GPU; never an error) */
int sdfk_device_count(void);
const char* sdfk_last_error(void);

/* ---- programs --------------------------------------------------------------------------------
 * A program is the lowered form of one expression tree: what the reference holds as nested Python
 * closures (cores/modifications.py:55-63 `modified_object`, cores/combine.py:129-138) plus the
 * Euclidean transform of every node (cores/transformations.py:232-242).
 *   code   : 2 words per instruction: {op | a<<8 | b<<16 | c<<24, parameter offset}
 *            (opcodes: aegolius_amd/csrc/sdfk_ops.def)
 *   params : fp32 parameter table (host-precomputed constants)
 *   tables : fp32 variable-length tables (poly-lines, point sets, convex pieces); may be NULL/0
 *   result_reg : value register that holds the field after the last instruction
 * The program is validated (opcodes, register indices, parameter ranges) — a malformed program is
 * rejected here, never launched. */
sdfk_program* sdfk_program_create(const uint32_t* code, size_t n_instr, const float* params, size_t n_params,
                                  const float* tables, size_t n_tables, int result_reg);
void sdfk_program_destroy(sdfk_program* prog);
/* Replace the parameter values of a program in place (same topology, new shape parameters). */
int sdfk_program_set_params(sdfk_program* prog, const float* params, size_t n_params);
/* Brick culling (optional, before first use of the program): n_sites rows (at most 32767) {combiner index, a_start,
 * a_end, b_start, b_end} naming, for min/max-type combiners, the instruction ranges that produce the
 * two operands, and k[i] = L_a + L_b, the sum of the Lipschitz constants of the operand fields with
 * respect to the input point. The specialised kernels then probe the tree per BRICK — 32 points x 16 grid rows when the
 * caller gives the row length (sdfk_eval_device_rows, grids), 128 consecutive points otherwise — and skip operand
 * subtrees that provably cannot change the result on that brick; results are bit-identical to the un-culled
 * evaluation. Sites whose ranges have side effects on registers read later are kept but never skipped.
 * How the sites are used: up to 64 of them as two mask bits each (the widest, in program order; the line-brick kernel
 * takes 31). The probe runs lane-parallel when every leaf range (a range without a site inside) reads nothing but the
 * input point: all leaves at all probe centres on the lanes of the workgroup, 8 / 4 / 1 centres per brick. A program
 * that holds an n-ary hard min / max over 17 to 32768 such leaves (CombineGeometry("UNION").combine(*many)) runs in
 * "chain mode" with all of the chain's sites: one function per kind of leaf, tables of parameter offsets, a list of
 * surviving leaves per brick; it builds in about a second whatever its size. The chain may be the whole program (with
 * value modifications of its result) or an operand of a small program around it — clipped, blended, subtracted: those
 * instructions (at most 64 + a quarter of the chain's, and 256) run per point around the chain's value, un-culled. */
int sdfk_program_set_cull(sdfk_program* prog, const uint32_t* sites, size_t n_sites, const float* k);
/* Members of the n-ary chain when the program runs in chain mode (after sdfk_program_set_cull), else 0. */
int sdfk_program_chain_members(const sdfk_program* prog);
/* Generated HIP source of the specialised kernel (for inspection / tests); NULL on error. */
const char* sdfk_program_source(sdfk_program* prog);
/* Compile the specialised kernel for gfx950 with hiprtc without needing a GPU (build check).
 * Returns 0 and the code-object size in *code_size. */
int sdfk_program_compile_check(sdfk_program* prog, size_t* code_size);
/* Kernel flavours: one hiprtc translation unit each, built only when a call needs it. */
#define SDFK_FLAVOUR_PLAIN_ARRAY 0 /* sdfk_spec_v4 / v1: straight-line body on a (3, n) array */
#define SDFK_FLAVOUR_PLAIN_GRID 1  /* the same from per-axis grid tables */
#define SDFK_FLAVOUR_TILE_ARRAY 2  /* exact culling on bricks of 128 consecutive points */
#define SDFK_FLAVOUR_TILE_GRID 3
#define SDFK_FLAVOUR_TILE_MASK 4   /* test aid (sdfk_debug_brick_masks) */
#define SDFK_FLAVOUR_ROWS_ARRAY 5  /* exact culling on blocks of 32 points x 16 grid rows (sdfk_eval_device_rows) */
#define SDFK_FLAVOUR_ROWS_GRID 6
#define SDFK_FLAVOUR_ROWS_MASK 7   /* test aid (sdfk_debug_row_masks) */
#define SDFK_FLAVOUR_ROWS2D_ARRAY 8 /* the row-block kernel built for flat grids (sdfk_eval_device_rows2d) */
#define SDFK_FLAVOUR_ROWS2D_GRID 9
#define SDFK_FLAVOUR_RAYS 10       /* sdfk_spec_rays / sdfk_spec_raycam: sphere tracing (sdfk_trace_rays_device /
                                      sdfk_trace_camera_device) around the straight-line body, one ray per lane; needs no
                                      cull sites and has no FLAGS / XY build. Not part of sdfk_program_compile_check. The
                                      kernels of RAYS and SPANS take (PRM, TAB, source, options, the march's outputs, STATS):
                                      csrc/sdfk_raydev.h, SDFK_MARCH_KERNEL; long chains get a culled pair (csrc/sdfk_raycull.h). */
#define SDFK_FLAVOUR_OCCUPANCY 11  /* sdfk_spec_occ_list / sdfk_spec_occ_all: the sample pass of sdfk_eval_grid_occupancy around
                                      the same body, one sub-sample per lane; as RAYS: no cull sites needed, no FLAGS / XY
                                      build, not part of sdfk_program_compile_check. */
#define SDFK_FLAVOUR_SPANS 12      /* sdfk_spec_spans / sdfk_spec_spancam: every crossing of a ray with the solid and its chord
                                      (sdfk_span_rays_device / sdfk_span_camera_device) around the same body; long chains get
                                      the culled pair as RAYS does. As RAYS: no cull sites needed, no FLAGS / XY build, not
                                      part of sdfk_program_compile_check. */
#define SDFK_FLAVOUR_SECONDARY 13  /* sdfk_spec_visibility / sdfk_spec_occlusion: the secondary marches (sdfk_visibility_rays_device /
                                      sdfk_occlusion_rays_device) around the same body, array rays only; long chains get a
                                      culled pair as RAYS does. As RAYS: no cull sites needed, no FLAGS / XY build, not part of
                                      sdfk_program_compile_check. */
#define SDFK_FLAVOUR_MOMENTS 14    /* sdfk_spec_mom_list / sdfk_spec_mom_all: the sample pass of sdfk_eval_grid_moments around the
                                      same body, one sub-sample per lane (csrc/sdfk_momdev.h); as OCCUPANCY: no cull sites
                                      needed, no FLAGS / XY build, not part of sdfk_program_compile_check. */
/* OR-ed onto a PLAIN / ROWS / ROWS2D flavour: its flag-writing build (one bit per point, value <= threshold, instead of
   the field — what sdfk_eval_device_select / sdfk_eval_grid_select launch). A translation unit of its own: the field
   kernels carry none of it (as a run-time branch it cost the 20-primitive tree 10 % at 1025^3). */
#define SDFK_FLAVOUR_FLAGS 0x100
/* OR-ed onto PLAIN_ARRAY / ROWS2D_ARRAY: the build for two-row coordinates (z = 0 by contract: sdfk_eval_device_rows2d_xy) */
#define SDFK_FLAVOUR_XY 0x200
/* Build (or fetch from the caches) ONE flavour, GPU or not: its code-object size and the seconds this call took. */
int sdfk_program_compile_flavour(sdfk_program* prog, int flavour, size_t* code_size, double* seconds);
/* Test aid: with enable != 0 every chain-mode row-block launch synchronises after the pre-pass of its candidate lists and
 * records { fine cells, coarse cells, pool entries used, pool capacity, sum of the fine lists' lengths, longest fine list,
 * fine cells without a list (their bricks probe every member), empty cells }; out8 (nullable) receives the record of the
 * last such launch and clears it. */
void sdfk_debug_cells_stats(int enable, long long* out8);
/* Test aid: with enable != 0 every launch of a culled ray kernel that was built with -DSDFK_DEBUG_RAYSTATS=1
 * (sdfk_debug_set_rtc_defs) is synchronised and its counters are added to a record; out8 (nullable) receives the record
 * and clears it: { list builds, member evaluations of those builds, survivor evaluations, plain-loop evaluations,
 * splits, point evaluations, 0, 0 }. Survivor and plain-loop evaluations are in lane slots — 64 per wave and evaluation,
 * whatever the number of marching lanes, as the hardware spends them: a list of n survivors adds 64 n to the third, a
 * group that ran every member 64 to the fourth; a point evaluation is one evaluation call of one wave. So
 * (builds' evaluations + survivor evaluations + members * plain-loop evaluations) / 64 per point evaluation is the number
 * of members a lane paid for per evaluation; in the plain kernel that is every member. */
void sdfk_debug_rays_stats(int enable, long long* out8);
/* Test aid: build one flavour the way BACKGROUND builds are run — in a child process (aegolius_amd/sdfk_rtc_helper,
 * csrc/sdfk_rtc_helper.c) — and return the code-object size; nothing is cached. While the interpreter kernel serves the
 * first calls of a new tree shape (SDFK_MODE_AUTO) the compiler never runs inside the calling process: hiprtc holds a
 * process-wide lock of its compiler library for the whole build, against which a dlopen of any HIP library on another
 * thread deadlocks. Without the helper next to the library there are no background builds: the first call waits. */
int sdfk_debug_compile_external(sdfk_program* prog, int flavour, size_t* code_size);
/* Wait until no background kernel build is queued or running. */
void sdfk_jit_drain(void);
/* The same for a process that is leaving: queued builds are dropped, running compiler child processes killed (a build of a
 * big tree takes up to a minute; nobody would use its kernel). What the Python layer registers with atexit. */
void sdfk_jit_cancel(void);
/* hiprtc builds this process has actually run (cache hits excluded) and the seconds they took. */
void sdfk_debug_jit_stats(int64_t* builds, double* seconds);
/* Extra -D switches handed to hiprtc for kernels built from now on (experiments; also env SDFK_RTC_DEFS). */
void sdfk_debug_set_rtc_defs(const char* defs);

/* ---- evaluation ------------------------------------------------------------------------------
 * Replaces GenericGeometry.create / propagate (cores/geom.py:29-60) for one whole tree:
 * out[i] = tree(co[0][i], co[1][i], co[2][i]).
 * d_co  : device pointer to a (3, n) fp32 array; row r starts at d_co + r*row_stride (elements).
 * d_out : device pointer to n fp32.
 * Uses 16-byte vector loads when d_co, d_out and row_stride allow (16-B aligned, stride % 4 == 0). */
int sdfk_eval_device(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, float* d_out,
                     void* stream, int mode);
/* The same with a LAYOUT HINT: the n points are consecutive rows of row_len points (n % row_len == 0) — for the
 * (3, N) array of generate_grid (cores/helper_functions.py:86-91, meshgrid "ij" flattened) row_len is the last
 * grid dimension. Brick culling then works on blocks of 32 points x 16 rows instead of 128 points in a line
 * (4x smaller bounding spheres, far fewer surviving subtrees), and rows need no 16-byte alignment. The hint
 * affects speed only: the field is bit-identical to sdfk_eval_device for ANY row_len (bounds, the "one x and
 * one y per row" test and every skip decision are derived from the coordinates actually read). */
int sdfk_eval_device_rows(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len,
                          float* d_out, void* stream, int mode);
/* The same with the second layout hint of a 3-D grid: the rows come in PLANES of plane_rows rows (the second grid
 * dimension; rows of one plane share x) and the first row of the array is row first_row_in_plane of its plane
 * (0 for a whole grid, anything for an x-slab of whole rows). Row blocks then never straddle two planes — such a
 * block spans the whole y extent of the grid and culls nothing (1 block in 32 at 513^3). plane_rows = 0: unknown
 * (= sdfk_eval_device_rows). Hints only: the field is bit-identical for any values. Honoured when the environment
 * sets SDFK_PLANE_BLOCKS=1: measured on 2^k + 1 grids the partial block that then ends every plane costs what the
 * straddling block saved, so by default the call equals sdfk_eval_device_rows. */
int sdfk_eval_device_rows3d(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len,
                            int64_t plane_rows, int64_t first_row_in_plane, float* d_out, void* stream, int mode);
/* The same for the array of a FLAT grid (generate_grid with two sizes, cores/helper_functions.py:63-75: rows run
 * along y, row_len = the second grid dimension, the z row is all zeros): the kernel is built so that the x part of
 * every root transform is computed once per row. Again a hint only — bricks whose z is not exactly 0 or whose x
 * varies along a row take the general path, and the field is bit-identical to sdfk_eval_device (up to the sign of
 * a zero). */
int sdfk_eval_device_rows2d(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len,
                            float* d_out, void* stream, int mode);
/* Flat grids WITHOUT their z row: d_xy is a (2, n) array — row 0 = x, row 1 = y, row pitch row_stride elements — and
 * z = 0 is the CONTRACT of the call, not something the kernel reads (the reference's 2-D generate_grid,
 * cores/helper_functions.py:63-75, always appends a row of zeros; streaming it costs a quarter of the traffic: 12
 * instead of 16 bytes per point). row_len as for sdfk_eval_device_rows2d (0: no layout hint — the plain kernel). The
 * field is bit-identical to sdfk_eval_device_rows2d on the same x, y with a zero z row. Waits for the specialised kernel
 * (the interpreter kernel has no two-row build): when that build is unavailable the call returns -3 in EVERY mode, nothing
 * launched, nothing written; programs that read auxiliary fields are refused. */
int sdfk_eval_device_rows2d_xy(sdfk_program* prog, const float* d_xy, int64_t n, int64_t row_stride, int64_t row_len,
                               float* d_out, void* stream, int mode);
/* Host-buffer convenience: stages co (dtype 0 = fp32, 1 = fp64; (3, n) with row stride in elements)
 * through device memory in chunks, evaluates and copies the fp32 field back. */
int sdfk_eval_host(sdfk_program* prog, const void* co, int co_dtype, int64_t n, int64_t row_stride, float* out,
                   int device, int mode);
/* Same staging of host coordinates, but the field is written to d_out — n floats of DEVICE memory on `device` —
 * and stays there for the field consumers below (nothing is copied back). */
int sdfk_eval_host_resident(sdfk_program* prog, const void* co, int co_dtype, int64_t n, int64_t row_stride,
                            float* d_out, int device, int mode);
/* Evaluate directly on a regular grid without materialising coordinates (4 B/point of traffic):
 * point `start + i` of the flat index n = (ix*n1 + iy)*n2 + iz takes (ax0[ix], ax1[iy], ax2[iz]).
 * Replaces generate_grid + create (cores/helper_functions.py:23-93). Axis tables are HOST pointers. */
int sdfk_eval_grid(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                   int64_t n2, int64_t start, int64_t count, float* d_out, void* stream, int mode);
/* Same, field copied back to a HOST buffer in device-sized chunks: the whole generate_grid + create round
 * trip without a coordinate array on either side. */
int sdfk_eval_grid_host(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                        const float* ax2, int64_t n2, int64_t start, int64_t count, float* out, int device, int mode);
/* Single-process multi-GPU: the grid is cut into n_shards contiguous slabs of whole rows (the remainder goes to
 * the last); shard d runs on devices[d] (devices == NULL: d modulo the device count), all shards concurrently,
 * each copying its slab into `out` (HOST, n0*n1*n2 floats). Slabs are independent (the path is pointwise): no
 * collective. The multi-process route (one rank per GPU, torch.distributed) is aegolius_amd/distributed.py. */
int sdfk_eval_grid_sharded(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                           const float* ax2, int64_t n2, int n_shards, const int* devices, float* out, int mode);
/* The same partition with the field left on the DEVICES: shard d runs on devices[d] and lands in its place of d_full, a
 * buffer of n0*n1*n2 floats on gather_device — in place for the shards of that device, by hipMemcpyPeerAsync (device to
 * device over xGMI, no host buffer) for the others. */
int sdfk_eval_grid_sharded_device(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                  const float* ax2, int64_t n2, int n_shards, const int* devices, int gather_device,
                                  float* d_full, int mode);
void sdfk_set_default_mode(int mode);
/* Test / diagnostics aid for brick culling: writes one 64-bit skip mask per brick of 128 consecutive
 * points (ceil(n / 2048) * 16 entries; bit 2k = first operand of site k skipped, bit 2k+1 = second operand,
 * bit 63 = all points of the brick share x and y). */
int sdfk_debug_brick_masks(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, uint64_t* d_masks,
                           void* stream);
/* The same for the row-block kernel of sdfk_eval_device_rows: 3 words per brick {skip bits of sites 0-31, of sites
 * 32-63, kind: 1 = every row segment has one x and one y, 0 = not}. Bricks are WINDOWS of 32 points aligned in the flat
 * array: window k of row r is line floor(r * row_len / 32) + k, so it starts up to 31 points before the row when
 * row_len is no multiple of 32; brick q covers window q % nchunk of rows [brick_rows * (q / nchunk), + brick_rows),
 * nchunk = row_len / 32 if that is exact, else (row_len + 62) / 32. With d_masks == NULL only *n_bricks and
 * *brick_rows are returned. */
int sdfk_debug_row_masks(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len,
                         uint64_t* d_masks, int64_t* n_bricks, int* brick_rows, void* stream);
/* Test aid: which kernel would an evaluation get? The plan of a request, computed on the host — no device is touched, so
 * it answers on a machine without one. request, 13 values:
 *   [0] source: 0 = a coordinate array, 1 = grid tables   [1] points (> 0)        [2] mode (SDFK_MODE_*)
 *   [3] rows and output 16-byte aligned (0 / 1)            [4] row_len hint        [5] flat hint (0 / 1)
 *   [6] plane_rows hint   [7] first_row_in_plane hint      [8] flags instead of the field: fused selection (0 / 1)
 *   [9] two-row coordinates (0 / 1)                        [10] n1, [11] n2, [12] start of a grid ([4]-[7] are an array's)
 * plan, 4 values: [0] the resolved mode (AUTO only where the call may start on the interpreter kernel; INTERPRET: no
 * kernel is built), [1] the SDFK_FLAVOUR_* a specialised launch takes, [2] 1 when the call has no interpreter fallback
 * (flags, two-row coordinates: -3 when the build is unavailable), [3] bricks of a row-block launch (0 for other flavours). */
int sdfk_debug_eval_plan(sdfk_program* prog, const int64_t* request, int64_t* plan);

/* ---- staged evaluation: grid-neighbourhood modifications ------------------------------------------
 * signed / conv_averaging / conv_edge_detection (cores/modifications.py:220-275, 1589-1637) reshape the field to
 * the grid and look at neighbours, so a tree that contains them is evaluated in stages: the sub-tree below the
 * operator with an ordinary program, the operator on the resident field (below), and the rest of the tree with a
 * program whose V_FIELD instructions read that field as auxiliary input c: d_aux + c*aux_stride + point index.
 * Programs with V_FIELD instructions must be run through the _aux entry points (the others refuse them). */
int sdfk_eval_device_aux(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, const float* d_aux,
                         int n_aux, int64_t aux_stride, float* d_out, void* stream, int mode);
int sdfk_eval_grid_aux(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                       int64_t n2, int64_t start, int64_t count, const float* d_aux, int n_aux, int64_t aux_stride,
                       float* d_out, void* stream, int mode);
/* Operators on a DEVICE field of n0*n1*n2 fp32 laid out like the (N,) output (flat index (i*n1 + j)*n2 + k; 2-D
 * fields: n2 = 1), in place, synchronous:
 *   box average  = post_processing.conv_averaging (cores/post_processing.py:561-600): scipy.ndimage.convolve with
 *                  ones(k0,k1,k2)/(k0*k1*k2), mode "reflect", `iterations` times;
 *   edge detect  = post_processing.conv_edge_detection (:603-623): [[-1,-1,-1],[-1,8,-1],[-1,-1,-1]] on axes 0, 1;
 *   signed       = ModifyObject.signed (cores/modifications.py:220-275): unchanged if the field has a negative value,
 *                  else boundary = field < sep_min (the smallest grid spacing), scan-line parity along axes 0 and 1,
 *                  2x2x1 average, inner crop + edge pad (crop = 0: signed_old, :163-218, without it),
 *                  field *= (1 - 2*(average > 0.5)). */
/* d_field: 16-byte aligned for sdfk_field_min (it reads 16-byte pieces); sdfk_grid_signed takes any float alignment. */
int sdfk_field_min(const float* d_field, int64_t n, float* out_min, void* stream);
/* d_scratch: n0*n1*n2*4 bytes of device memory for the operator's work arrays (NULL: allocated and freed inside).
 * sdfk_grid_signed keeps its work as bit planes (six arrays of n0*n1*ceil(n2/32) words) inside it and allocates its
 * own few bytes for grids thinner than 11 points along the last axis. */
int sdfk_grid_box_average(float* d_field, int64_t n0, int64_t n1, int64_t n2, int k0, int k1, int k2, int iterations,
                          void* d_scratch, void* stream);
int sdfk_grid_edge_detect(float* d_field, int64_t n0, int64_t n1, int64_t n2, void* d_scratch, void* stream);
int sdfk_grid_signed(float* d_field, int64_t n0, int64_t n1, int64_t n2, float sep_min, int crop, void* d_scratch,
                     void* stream);
/* Test aid (host only, launches nothing): which box kernel sdfk_grid_box_average would run for this grid and kernel
 * (sdfk_grid_edge_detect: k = 3, 3, 1). The launch reads the same decision. out8 = { flags: 1 = marching kernel
 * (else the tiled one), 2 = FAST reflection (kernel at most twice the field), 4 = flat field relabelled (1, n0, n1);
 * K0C (marching kernel, else 0); K2C (0 = run-time k2); marching: planes per segment, tiled: halo planes per LDS chunk;
 * LDS chunks per output (marching: 1); the launch grid x, y, z }. Honours SDFK_BOX_NO_MARCH and SDFK_BOXM_SEG. */
int sdfk_debug_box_variant(int64_t n0, int64_t n1, int64_t n2, int k0, int k1, int k2, int* out8);
/* `signed` on ONE SLAB of a grid that is sharded over several GPUs: the scan lines cross every slab, but all they
 * read is one bit per point (field < sep_min). sdfk_grid_boundary_mask writes that test for n points as bytes; the
 * ranks exchange the bytes (aegolius_amd/distributed.py); sdfk_grid_signed_slab runs the scans on the WHOLE grid's
 * mask (n0 * n1 * n2 bytes) and flips the sign of the planes [plane0, plane0 + planes) held in d_slab. The "already
 * signed" test of the reference (modifications.py:236-237) is the caller's, as a minimum over all ranks. */
int sdfk_grid_boundary_mask(const float* d_field, int64_t n, float sep_min, unsigned char* d_mask, void* stream);
int sdfk_grid_signed_slab(float* d_slab, int64_t plane0, int64_t planes, const unsigned char* d_mask, int64_t n0, int64_t n1,
                          int64_t n2, int crop, void* d_scratch, void* stream);

/* ---- consumers of a resident field -------------------------------------------------------------
 * What the reference does with the (N,) field right after create(), on the device, synchronous:
 *   select    = the mask of GenericGeometry.point_cloud (cores/geom.py:62-74): the indices i, ascending, with
 *               field[i] <= threshold (NaN never selected). *count always receives the size of the selection;
 *               d_index == NULL counts only; otherwise d_index (DEVICE, capacity entries) must hold the selection.
 *               d_scratch: sdfk_field_select_scratch(n) bytes (about n / 8) of 8-byte-aligned device memory (NULL:
 *               allocated and freed inside). The field is read once: the count pass leaves 4 flag bits per quad in
 *               the scratch, the scatter pass works from those.
 *               d_field must be 16-byte aligned.
 *   gradient  = vector_functions.from_sdf (cores/vector_functions.py:130-140): numpy.gradient with unit spacing
 *               (central differences, one-sided on the faces) over the LAST ncomp axes of the (n0, n1, n2) field
 *               (the others must have length 1; every differentiated axis needs >= 2 points), then, if
 *               normalize != 0, batch_normalize (cores/vector_modification_functions.py:14-20): each vector divided
 *               by its norm unless the norm is 0. fp32 arithmetic: the raw gradient (normalize == 0) equals
 *               numpy's float64 result rounded to fp32, the direction is within 1e-6 per component. Row r of
 *               d_vec (DEVICE, ncomp rows of row_stride floats) is the derivative along axis 3 - ncomp + r;
 *               d_field, d_vec and row_stride * 4 must be 16-byte aligned. */
size_t sdfk_field_select_scratch(int64_t n);
/* Second half of a selection whose count-only call (d_index == NULL, caller-owned d_scratch) has just run on a field
 * of n points: writes the `count` indices that call announced without reading the field again. */
int sdfk_field_select_finish(int64_t n, int64_t count, int64_t* d_index, int64_t capacity, void* d_scratch, void* stream);

/* FUSED selection (GenericGeometry.point_cloud, cores/geom.py:62-74, without a field): the evaluation kernels write one
 * bit per point — field <= threshold — instead of the field (12 B/point of coordinates in, 1/8 B/point out), and count,
 * scan and scatter work on those flags alone; the indices are numpy.flatnonzero(tree(co) <= threshold), ascending, and
 * the bits are those of sdfk_eval_device's field. Same two-step protocol as sdfk_field_select: d_index == NULL returns
 * the count and keeps the flags in d_scratch (sdfk_eval_select_scratch(n, row_len) bytes of device memory, 8-byte aligned) for
 * sdfk_eval_select_finish. row_len / flat: the layout hints of sdfk_eval_device_rows / _rows2d (0: none). Runs on the
 * specialised kernels (the call waits for their build, and returns -3 in EVERY mode when that build is unavailable: the
 * interpreter kernel writes no flags); programs with auxiliary fields are refused. */
size_t sdfk_eval_select_scratch(int64_t n, int64_t row_len);
int sdfk_eval_device_select(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len, int flat,
                            float threshold, int64_t* d_index, int64_t capacity, int64_t* count, void* d_scratch,
                            void* stream, int mode);
int sdfk_eval_grid_select(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                          int64_t n2, int64_t start, int64_t count_points, float threshold, int64_t* d_index,
                          int64_t capacity, int64_t* count, void* d_scratch, void* stream, int mode);
/* row_len, mode: as in the count-only call before it (grids: the last grid dimension longer than one point when the range
 * starts at a row boundary, else 0) — they decide how the flags are laid out. */
int sdfk_eval_select_finish(sdfk_program* prog, int64_t n, int64_t row_len, int mode, int64_t count, int64_t* d_index,
                            int64_t capacity, void* d_scratch, void* stream);
int sdfk_field_select(const float* d_field, int64_t n, float threshold, int64_t* d_index, int64_t capacity,
                      int64_t* count, void* d_scratch, void* stream);
int sdfk_field_gradient(const float* d_field, int64_t n0, int64_t n1, int64_t n2, int ncomp, int normalize,
                        float* d_vec, int64_t row_stride, void* stream);

/* ---- liquid-crystal waveguide fields ------------------------------------------------------------
 * cores/vector_functions_special.py on DEVICE fields of n0*n1*n2 fp32 (flat index (i*n1 + j)*n2 + k), synchronous,
 * float64 arithmetic in numpy's order from the fp32 inputs:
 *   crossings = compute_crossings_2d (:14-36) of grid plane k = 0: of d_uu, or, when d_ww != NULL, of
 *               pp = sqrt((2uu/w)^2 + (ww/d)^2). m = min of the plane; c1[i, j] = isclose(s[i, j], m, atol=thr) &
 *               !isclose(s[i, j-1], m, atol=thr) for j >= 1 (rtol 1e-5 as numpy's default); parity of the running
 *               count along j; conv_averaging(parity, 5, 2) >= 0.5 (reflect mode). d_sign (DEVICE, n0*n1 int8)
 *               receives +-1. Bit-identical to the reference on fp32-representable inputs.
 *   lcwg      = lcwg1_2d (variant 0, :127-161: raw numpy.gradient of uu turned about z by phis, normalised),
 *               lcwg1_p1 (1, :164-207) and lcwg1_m1 (2, :210-251): normalised gradient of pp, turned about
 *               e2 = vec x e1 by phis, then about e1 = |(-vec_y, vec_x, 0)| by -2 alpha, alpha = +-arctan2(2ww/d^2,
 *               8uu/w^2), normalised; phis = sign * (clip(value, 0, 1) pi + pi/2), value = 2uu/w (2D) or pp.
 *               sign_kind 0: sign = sign_value everywhere; 1: d_sign is the int8 plane of sdfk_field_crossings_2d
 *               (point p takes entry p / n2); 2: d_sign holds one fp32 number per point. Every axis needs >= 2
 *               points; d_ww may be NULL for variant 0. d_vec: three rows of row_stride floats. 20 B/point of traffic
 *               for variants 1 and 2 (uu, ww in, 3 rows out), 16 for variant 0.
 *   lcwg old  = lcwg1_2d_old / lcwg1_p1_old / lcwg1_m1_old (:39-124), pointwise: d_r holds three rows of r_stride
 *               floats (the positions r), d_uu n numbers. */
int sdfk_field_crossings_2d(const float* d_uu, const float* d_ww, int64_t n0, int64_t n1, int64_t n2, double w, double d,
                            double thr, signed char* d_sign, void* stream);
int sdfk_lcwg_eval(int variant, const float* d_uu, const float* d_ww, int64_t n0, int64_t n1, int64_t n2, double w, double d,
                   int sign_kind, double sign_value, const void* d_sign, float* d_vec, int64_t row_stride, void* stream);
int sdfk_lcwg_old_eval(int variant, const float* d_r, int64_t r_stride, const float* d_uu, int64_t n, double w, double d,
                       float* d_vec, int64_t row_stride, void* stream);

/* ---- vector-field programs ----------------------------------------------------------------------
 * The reference's vector-field path (cores/geom.py:213-362 VectorField; cores/vector_functions.py:15-127 field
 * definitions; cores/modifications.py:1666-1975 ModifyVectorObject; cores/vector_modification_functions.py:14-160)
 * as ONE pointwise kernel: instruction 0 turns the input triple p into a vector, the others are the modifications
 * in the order they were applied. op = opcode | kindA << 8 | kindB << 12; kinds: 0 none, 1 number (imm[0] for A,
 * imm[3] for B), 2 3-vector (imm[0..2]), 3 one row of `streams` (src = row index: a per-point number), 4 three rows
 * (src = first row: a per-point vector), 5 the input triple p itself (revolutions about the axes of the same
 * coordinates). Opcodes (A / B operands):
 *   0 p itself | 1 (r, phi, theta) = p | 2 (r, phi, z) = p | 3 p/|p| | 4 (x, y, 0)/|(x, y)| | 5 vortex |
 *   6 radial-cylindrical turned by A | 7 vortex turned by A | 8 constant A | 9 rows A                (initialisers)
 *   10 v + A | 11 v - A | 12 v * A | 13 turn about z by A | 14 about x | 15 about y | 16 polar turn by A |
 *   17 turn about axis A by angle B | 18 / 19 / 20 revolve about x / y / z with coordinates A | 21 normalise.
 * out_kind: 0 the vector (3 rows) | 1 x | 2 y | 3 z | 4 atan2(y, x) | 5 acos(z) | 6 length (1 row).
 * fp32 arithmetic; zero vectors stay zero under normalisation. Asynchronous on `stream` (device flavour). */
typedef struct {
    int32_t op;
    int32_t src[2];
    float imm[4];
} sdfk_vec_instr;
/* d_p, d_out: 16-byte aligned, row strides multiples of 4 floats; d_streams: n_streams rows of stream_stride floats. */
int sdfk_vec_eval_device(const sdfk_vec_instr* prog, int n_instr, const float* d_p, int64_t n, int64_t p_stride,
                         const float* d_streams, int n_streams, int64_t stream_stride, int out_kind, float* d_out,
                         int64_t out_stride, void* stream);
/* By default a chain's TOPOLOGY (opcodes, operand kinds, stream rows, read-out) is compiled once per process with
 * hiprtc into a straight-line kernel (immediates stay run-time values); sdfk_vec_set_interpret(1) — or
 * SDFK_VEC_INTERPRET=1 in the environment — runs the interpreter kernel instead. Both give the same bits.
 * sdfk_vec_source: the generated HIP source (valid until the next call on the thread); sdfk_vec_compile_check:
 * compile it for gfx950 without a device. */
void sdfk_vec_set_interpret(int on);
const char* sdfk_vec_source(const sdfk_vec_instr* prog, int n_instr, int n_streams, int out_kind);
int sdfk_vec_compile_check(const sdfk_vec_instr* prog, int n_instr, int n_streams, int out_kind, size_t* code_size);
/* HOST arrays staged through the device in chunks: p (dtype 0 = fp32, 1 = fp64; (3, n) contiguous) or, when ax0..ax2
 * are given, the generate_grid cloud of those tables (expanded on the device); streams (n_streams, n) fp32; out (3, n)
 * or (n,) fp32. */
int sdfk_vec_eval_host(const sdfk_vec_instr* prog, int n_instr, const void* p, int p_dtype, int64_t n, const float* ax0,
                       int64_t n0, const float* ax1, int64_t n1, const float* ax2, int64_t n2, const float* streams,
                       int n_streams, int out_kind, float* out, int device);

/* ---- grid builder -----------------------------------------------------------------------------
 * numpy.linspace(lo, hi, n) in float64 (step = (hi-lo)/(n-1); y[i] = i*step + lo; y[n-1] = hi),
 * rounded to fp32 — the per-axis table of generate_grid (cores/helper_functions.py:56-88). */
int sdfk_linspace_f32(double lo, double hi, int64_t n, float* out);
/* ---- nearest-point tables ---------------------------------------------------------------------
 * Box tree over a point table for the nearest-point leaves (point clouds, resampled / parametric curves, curve
 * instancing: C/sdf_2D.py:221-224, C/sdf_3D.py:283-286 build a scipy KDTree per evaluation; here the tree is part of the
 * program's tables, built once per lowering). Host only, no GPU. pts: (m, 3) fp32, row-major; leaf: points per leaf box
 * = children per box on every level above (the lowering uses 32); table: out — root boxes, middle boxes, leaf boxes (8
 * floats each: lo, hi, first child, children), then the points in leaf order —, capacity table_cap floats (3 m + 24 (m /
 * (leaf / 2) + 4) always suffices); order: out or NULL, the original index of every point in leaf order; n_root /
 * point_base: out, the number of root boxes and the offset of the first point. Returns the number of floats written,
 * < 0 on error (-2: more than 2^24 words — table indices are carried as fp32). */
int64_t sdfk_point_tree_build(const float* pts, int64_t m, int leaf, float* table, int64_t table_cap, int64_t* order,
                              int64_t* n_root, int64_t* point_base);

/* Fill a device (3, count) coordinate slab for flat indices [start, start+count) of the grid. */
int sdfk_grid_fill(float* d_co, int64_t row_stride, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                   const float* ax2, int64_t n2, int64_t start, int64_t count, void* stream);

/* ---- device memory / timing plumbing (so callers need no HIP binding of their own) ------------ */
int sdfk_set_device(int device);
void* sdfk_malloc(size_t bytes);
int sdfk_free(void* d_ptr);
int sdfk_memcpy_h2d(void* d_dst, const void* src, size_t bytes);
int sdfk_memcpy_d2h(void* dst, const void* d_src, size_t bytes);
int sdfk_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes);
int sdfk_sync(void* stream);
void* sdfk_event_create(void);
int sdfk_event_destroy(void* ev);
int sdfk_event_record(void* ev, void* stream);
int sdfk_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms); /* synchronises on ev_stop */
/* plain (3,n)->(n) streaming kernel out = x+y+z with the same access pattern: measured HBM ceiling */
int sdfk_stream_probe(const float* d_co, int64_t n, int64_t row_stride, float* d_out, void* stream);


/* ---- forward-mode derivatives (dual numbers; csrc/sdfk_dual.inc, rules in csrc/sdfk_dualdev.h) ---------------------
 * A program is evaluated on dual numbers: next to its value, K = 1..4 tangents per point. Parameter mode: d_dparams holds
 * K rows of n_params floats (the program's parameter count), row k = d P / d theta_k; the coordinates carry no tangent.
 * Point mode (seed_points = 1, K = 3): the input point's tangents are the unit vectors, d_dparams is K rows of zeros,
 * and the tangents are the spatial gradient. d_value: n floats; d_tangent: K rows of tangent_stride floats.
 * Every instruction is evaluated (no culling, no code specialisation). */
/* 1 if opcode op has a dual rule, else 0 (the single table in csrc/sdfk_dualdev.h) */
int sdfk_dual_has_rule(int op);
/* 0: the program can be differentiated; 1: instruction *first_bad_op has no dual rule; 2: its register files exceed the
 * dual kernel's (16 coordinate / 8 value registers); < 0 on error. sdfk_last_error names the cause. */
int sdfk_program_jvp_check(sdfk_program* prog, int* first_bad_op);
int sdfk_eval_jvp_device(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, const float* d_dparams, int k,
                         int seed_points, float* d_value, float* d_tangent, int64_t tangent_stride, void* stream);
/* One value operation (a V_V opcode with a dual rule, P its parameter block) on n (value, tangent) pairs: the chain rule
 * through a post-processing map, parameter tangents zero. */
int sdfk_value_jvp_device(int op, const float* P, const float* d_v, const float* d_t, int64_t n, float* d_out_v,
                          float* d_out_t, void* stream);

/* ---- projection onto a level set (aegolius_amd.surface; csrc/sdfk_project.inc) ---------------------------------------
 * Newton iteration q <- q - relax (f(q) - level) grad f(q) / |grad f(q)|^2 from every input point, value and gradient from
 * the dual kernel's point mode, all iterations in one launch. Per point: d_q (3 rows q_stride apart) the final point,
 * d_value the field there, d_grad (3 rows grad_stride apart, may be null) its gradient there, d_start (may be null) the
 * field at the input point, d_info = status | iterations << 8. Status: 0 converged (|f - level| <= tol), 1 max_iter
 * steps taken without converging, 2 stalled (|grad f|^2 < 1e-24), 3 the field is not finite. A point that stops keeps
 * the q it had. max_iter 0 .. 255, tol >= 0, relax in (0, 1], level finite. Programs: those sdfk_program_jvp_check
 * accepts. Asynchronous on the stream; n == 0 launches nothing. */
int sdfk_project_points_device(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, float level, float tol,
                               int max_iter, float relax, float* d_q, int64_t q_stride, float* d_value, float* d_grad,
                               int64_t grad_stride, float* d_start, int32_t* d_info, void* stream);
/* The same launch, which also ADDS to d_wg_trips[w] the program evaluations of every wave of workgroup w
 * (sdfk_project_workgroups(n) counters, zeroed by the caller): what the iteration cost, for measurements. */
int64_t sdfk_project_workgroups(int64_t n);
int sdfk_project_points_counted_device(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, float level,
                                       float tol, int max_iter, float relax, float* d_q, int64_t q_stride, float* d_value,
                                       float* d_grad, int64_t grad_stride, float* d_start, int32_t* d_info,
                                       uint32_t* d_wg_trips, void* stream);

/* ---- reverse-mode derivatives (adjoint; csrc/sdfk_adjoint.inc, rules derived from csrc/sdfk_dualdev.h) --------------
 * One pass evaluates the program at n points with a restore tape and back-propagates a cotangent c_i per point; the
 * parameter adjoints P̄_j = sum_i c_i d f_i / d P_j are reduced on the device in float64 (deterministic order).
 * mode 0: d_in holds the cotangent c (n floats). mode 1 (sum of squares): d_in holds a target t (n floats), the cotangent
 * is 2 (f_i - t_i) and *h_loss receives sum_i (f_i - t_i)^2 (float64). d_out_value (n floats) and h_loss may be null.
 * h_pbar receives n_params doubles. flags bit 0: generic rules only (every product derived from the dual rule). Host
 * pointers h_pbar / h_loss are written before the call returns (the call waits for its stream). */
/* 0: the program can be back-propagated; 1 / 2: as sdfk_program_jvp_check; 3: its restore tape exceeds the kernel's
 * (*tape_floats receives its size in floats per point); 4: more parameters than the kernel's accumulator holds. */
int sdfk_program_vjp_check(sdfk_program* prog, int* first_bad_op, int64_t* tape_floats);
/* the adjoint kernel's limits: restore-tape floats per point, parameters per program */
int sdfk_vjp_limits(int* tape_floats, int* max_params);
int sdfk_eval_vjp_device(sdfk_program* prog, const float* d_co, int64_t n, int64_t row_stride, const float* d_in, int mode,
                         int flags, float* d_out_value, double* h_pbar, double* h_loss, void* stream);

/* ---- point cloud -> voxel occupancy (Points.to_image; csrc/sdfk_points.inc) ------------------------------------------
 * The grid is rx * ry * rz bytes, C order. d_cloud: (3, n) float64 rows row_stride apart; d_edges: the float64 bin
 * edges of the three axes back to back (rx + 1, ry + 1, rz + 1 values, numpy.histogramdd's). sdfk_points_bin zeroes the
 * grid and writes 1 into every voxel that holds a point (numpy's outliers and NaN dropped). sdfk_points_extent writes
 * rx + ry + rz "plane holds a voxel" bytes (x planes, then y, then z; rz <= 65536). sdfk_points_fill makes planes
 * [lo, hi) of axis 0 / 1 / 2 copies of plane src (src outside the range). sdfk_points_widen writes the grid as 0.0 / 1.0:
 * kind 0 float64, kind 1 float32. All four are asynchronous on the stream. */
int sdfk_points_bin(const double* d_cloud, int64_t n, int64_t row_stride, const double* d_edges, int64_t rx, int64_t ry,
                    int64_t rz, unsigned char* d_grid, void* stream);
int sdfk_points_extent(const unsigned char* d_grid, int64_t rx, int64_t ry, int64_t rz, unsigned char* d_flags, void* stream);
int sdfk_points_fill(unsigned char* d_grid, int64_t rx, int64_t ry, int64_t rz, int axis, int64_t src, int64_t lo, int64_t hi,
                     void* stream);
int sdfk_points_widen(const unsigned char* d_grid, int64_t n, int kind, void* d_out, void* stream);

/* ---- isosurface and contour extraction (aegolius_amd.mesh; csrc/sdfk_mesh.inc) ----------------------------------------
 * d_field: the (n0, n1, n2) field in C order (2-D: (n0, n1)), DEVICE, 16-byte aligned. ax0 .. ax2: HOST tables of the
 * axis coordinates (as sdfk_eval_grid_select takes them), each strictly increasing with at least 2 points. A point is
 * inside if field <= level (NaN outside; a NaN level is refused). One vertex per grid edge whose ends differ, numbered by
 * (owning lower point, axis); triangles (segments) by (cell, case-table order), counter-clockwise seen from outside
 * (segments: inside on the left). The exact definition is that of aegolius_amd/mesh.py.
 * Two steps, as sdfk_field_select: the counting call reads the field once, leaves its state in d_scratch (*_scratch bytes,
 * 256-byte aligned device memory) and returns the counts; *_finish writes the vertices (float32, 3 or 2 per vertex) and
 * the faces (3 or 2 vertex ids per entry, face_bytes 4 = int32, needs fewer than 2^31 vertices, or 8 = int64) up to the
 * given capacities, which must hold the counts. finish takes the same field, shape and level. */
size_t sdfk_field_isosurface_scratch(int64_t n0, int64_t n1, int64_t n2);
int sdfk_field_isosurface(const float* d_field, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                          int64_t n2, float level, int64_t* n_vertices, int64_t* n_faces, void* d_scratch, void* stream);
int sdfk_field_isosurface_finish(const float* d_field, int64_t n0, int64_t n1, int64_t n2, float level, int64_t n_vertices,
                                 int64_t n_faces, float* d_vertices, int64_t vertex_capacity, void* d_faces,
                                 int64_t face_capacity, int face_bytes, void* d_scratch, void* stream);
size_t sdfk_field_contour2d_scratch(int64_t n0, int64_t n1);
int sdfk_field_contour2d(const float* d_field, const float* ax0, int64_t n0, const float* ax1, int64_t n1, float level,
                         int64_t* n_vertices, int64_t* n_segments, void* d_scratch, void* stream);
int sdfk_field_contour2d_finish(const float* d_field, int64_t n0, int64_t n1, float level, int64_t n_vertices,
                                int64_t n_segments, float* d_vertices, int64_t vertex_capacity, void* d_segments,
                                int64_t segment_capacity, int segment_bytes, void* d_scratch, void* stream);
/* The same meshes of a PROGRAM on the grid of the axis tables, without a field or a coordinate array: the evaluation
 * kernels write one inside bit per point (their flag builds, as sdfk_eval_grid_select), and the finishing call evaluates
 * the program again only at the two ends of every crossing edge. Output identical to evaluating the grid to a field
 * (sdfk_eval_grid) and calling sdfk_field_isosurface / _contour2d on it. Same two steps and output buffers; d_scratch:
 * *_scratch bytes (at most 1 byte per grid point plus O(n0 + n1 + n2 + n / 8192)), 256-byte aligned. The finishing call
 * takes the tables, level and mode of the counting call; while it runs it allocates 32 bytes per vertex for the edge
 * ends and their values. Programs with auxiliary fields (staged) are refused: evaluate them to a field first. */
size_t sdfk_eval_grid_isosurface_scratch(int64_t n0, int64_t n1, int64_t n2);
int sdfk_eval_grid_isosurface(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                              int64_t n2, float level, int64_t* n_vertices, int64_t* n_faces, void* d_scratch, void* stream,
                              int mode);
int sdfk_eval_grid_isosurface_finish(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                     const float* ax2, int64_t n2, float level, int64_t n_vertices, int64_t n_faces,
                                     float* d_vertices, int64_t vertex_capacity, void* d_faces, int64_t face_capacity,
                                     int face_bytes, void* d_scratch, void* stream, int mode);
size_t sdfk_eval_grid_contour2d_scratch(int64_t n0, int64_t n1);
int sdfk_eval_grid_contour2d(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1, float level,
                             int64_t* n_vertices, int64_t* n_segments, void* d_scratch, void* stream, int mode);
int sdfk_eval_grid_contour2d_finish(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1, float level,
                                    int64_t n_vertices, int64_t n_segments, float* d_vertices, int64_t vertex_capacity,
                                    void* d_segments, int64_t segment_capacity, int segment_bytes, void* d_scratch,
                                    void* stream, int mode);
/* Plane stacks: the contours of a PROGRAM on every layer of the grid (heights, u, v) — `layers` >= 1 heights, nu >= 2 and
 * nv >= 2 in-plane values, all strictly increasing; point (l, i, j) is the program at (heights[l], u[i], v[j]), x from
 * the slowest axis as everywhere. Layer l is what sdfk_eval_grid_contour2d gives on the 2-D field of that layer with
 * axes (u, v), bit for bit; the stack's vertices (V, 2) float32 as (a, b) and segments (S, 2) are the layers' one after
 * the other, vertex ids global; offsets[l] .. offsets[l + 1] is layer l's range (layers + 1 entries, host arrays).
 * Same two steps as the contour calls: the counting call (evaluation to inside bits, count, scans, layer offsets) returns
 * V and S, the finishing call takes level and mode of the counting call, writes the arrays (segment_bytes 4 or 8 per
 * index) and copies the offsets out; while it runs it allocates 32 bytes per vertex. d_scratch: *_scratch bytes (at most
 * 1 byte per grid point plus O(layers + nu + nv + n / 8192)), 256-byte aligned.
 * sdfk_eval_grid_slices_measure does both steps in device memory it allocates and frees, then reduces every layer with
 * one workgroup, in float64 from the float32 vertices relative to the rectangle's centre (ca, cb) and in a fixed order
 * (no atomics): measures[6 l ..] = area (half the sum of t_s = (a0 - ca)(b1 - cb) - (a1 - ca)(b0 - cb) over the segments
 * (a0, b0) -> (a1, b1)), perimeter (sum of hypot), first moments (sum of (a0 + a1 - 2 ca) t_s / 6 and the same in b),
 * the number of segments, and the number of vertices on the border of the rectangle (a == u[0] or u[nu - 1], or
 * b == v[0] or v[nv - 1]: the contour leaves the grid there). Only the measures and the offsets come back.
 * Programs with auxiliary fields (staged) are refused. */
size_t sdfk_eval_grid_slices_scratch(int64_t layers, int64_t nu, int64_t nv);
int sdfk_eval_grid_slices(sdfk_program* prog, const float* heights, int64_t layers, const float* u, int64_t nu, const float* v,
                          int64_t nv, float level, int64_t* n_vertices, int64_t* n_segments, void* d_scratch, void* stream,
                          int mode);
int sdfk_eval_grid_slices_finish(sdfk_program* prog, int64_t layers, int64_t nu, int64_t nv, float level, int64_t n_vertices,
                                 int64_t n_segments, float* d_vertices, int64_t vertex_capacity, void* d_segments,
                                 int64_t segment_capacity, int segment_bytes, int64_t* vertex_offsets,
                                 int64_t* segment_offsets, void* d_scratch, void* stream, int mode);
int sdfk_eval_grid_slices_measure(sdfk_program* prog, const float* heights, int64_t layers, const float* u, int64_t nu,
                                  const float* v, int64_t nv, float level, double* measures, int64_t* vertex_offsets,
                                  int64_t* segment_offsets, void* d_scratch, void* stream, int mode);

/* ---- topology: connected components, cell counts, label fields (aegolius_amd.topology; csrc/sdfk_topology.inc) --------
 * Grid: D = 2 or 3 strictly increasing HOST axis tables of at least 2 points each, points in C order (flat index
 * p = (i0 n1 + i1) n2 + i2, as the mesh calls); n2 = 1 is a 2-D grid (ax2 is then not read). At most 2^31 - 1 points:
 * labels are int32. A point is inside iff f <= level, compared as selection keys — the mesh's rule, NaN outside. `region`:
 * SDFK_REGION_INSIDE labels the inside points, SDFK_REGION_OUTSIDE all the others. `connectivity`: SDFK_CONNECT_FACES joins
 * the 4 (2-D) / 6 (3-D) neighbours across a grid edge, SDFK_CONNECT_FULL the 8 / 26 neighbours of the surrounding block.
 * The canonical name of a component is the smallest flat index among its points (`first`); components are numbered
 * 0 .. K - 1 by ascending `first`, so every output is independent of scheduling. d_labels: n0 n1 n2 int32, DEVICE: the id
 * of the point's component, -1 where the point is not in the region.
 * Two steps, as the mesh calls. The labelling call makes the inside bits (sdfk_field_label: from a resident field;
 * sdfk_eval_grid_label: the flag builds of the evaluation kernels, no field, `mode` as for sdfk_eval_grid_isosurface),
 * labels them (init from the bits, lock-free union by atomicMin, compress, number; every phase a launch of its own) and
 * returns *count = K. sdfk_label_bits labels the inside bits a previous call left in the scratch — any of the labelling
 * or cell-count calls on the same grid — again, with another region or connectivity, without a second evaluation.
 * sdfk_label_finish, after a labelling call with the same d_labels and scratch, writes the K records to HOST arrays:
 * first[K] and sizes[K] (points) int64, lower[K D] and upper[K D] int32 (the index bounding box, D entries per record),
 * border[K] int32 (1 when a point of the component lies on a face of the grid); integer atomics only, so the records
 * do not depend on the order of the waves. It allocates 24 + 8 D bytes per component while it runs.
 * sdfk_field_cell_counts / sdfk_eval_grid_cell_counts: counts[4] (HOST) = V, E, F, C — the inside points, the grid edges
 * with both ends inside, the grid squares with all 4 corners inside, the grid cubes with all 8 corners inside (0 in
 * 2-D): the cells of the cubical complex the inside points span, Euler characteristic V - E + F - C. They leave the
 * inside bits in the scratch (sdfk_label_bits).
 * sdfk_label_field: d_out[p] = inside where d_labels[p] is an id with keep[id] != 0 (keep: HOST, count bytes), outside
 * elsewhere; n floats, one kernel.
 * sdfk_label_moments: the integer moments of every component, from the label array alone (16-byte aligned; any array of
 * -1 and ids below `count` on that grid will do, no scratch of a labelling is needed). sums: HOST, count rows of uint64,
 *     3-D: N, I0, I1, I2, I00, I01, I02, I11, I12, I22        2-D: N, I0, I1, I00, I01, I11
 * the sums of 1, i_a and i_a i_b (i_a the index on axis a) over the points whose label is the row's id. One pass over
 * the labels, row runs in closed form, 64-bit integer adds only: the rows do not depend on the order of the waves. It
 * allocates 80 (2-D: 48) bytes per component while it runs. d_scratch is not used (the labels are walked directly): pass
 * NULL. count = 0 returns at once. -2 and no launch: points x (longest axis - 1)^2 >= 2^63, a grid on which a sum could
 * wrap; -7: a label below -1 or not below count was met — such labels are left out, never used as an index.
 * d_scratch: sdfk_label_scratch bytes, 256-byte aligned: the inside bits, the region's bits, root flags and prefixes —
 * at most 1 byte per point plus O(n0 + n1 + n2 + n / 8192); with the labels 5 bytes per point. pass_ms (nullable):
 * SDFK_LABEL_PASSES floats that receive device-event milliseconds of bits (the region's complement included), init,
 * merge, compress, number. Every chase and retry loop on the device carries an iteration cap of n0 n1 n2; a call that
 * reaches it returns -7 (the algorithm cannot: labels only decrease — the cap turns a defect into an error, not a hang).
 * -1 and no launch: a NULL pointer, a misaligned field (16 bytes) or scratch, an axis of fewer than 2 points or not
 * strictly increasing, more than 2^31 - 1 points, a NaN level, an unknown connectivity or region, a scratch that does not
 * hold the bits (or the labelling) of that grid. Programs with auxiliary fields (staged) are refused: evaluate them to
 * a field first. Synchronous: the stream is idle on return. */
#define SDFK_CONNECT_FACES 0
#define SDFK_CONNECT_FULL 1
#define SDFK_REGION_INSIDE 0
#define SDFK_REGION_OUTSIDE 1
#define SDFK_LABEL_PASSES 5
size_t sdfk_label_scratch(int64_t n0, int64_t n1, int64_t n2);
int sdfk_field_label(const float* d_field, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                     int64_t n2, float level, int connectivity, int region, int32_t* d_labels, int64_t* count,
                     void* d_scratch, float* pass_ms, void* stream);
int sdfk_eval_grid_label(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                         int64_t n2, float level, int connectivity, int region, int32_t* d_labels, int64_t* count,
                         void* d_scratch, float* pass_ms, void* stream, int mode);
int sdfk_label_bits(int64_t n0, int64_t n1, int64_t n2, int connectivity, int region, int32_t* d_labels, int64_t* count,
                    void* d_scratch, float* pass_ms, void* stream);
int sdfk_label_finish(int64_t n0, int64_t n1, int64_t n2, int64_t count, const int32_t* d_labels, int64_t* first,
                      int64_t* sizes, int32_t* lower, int32_t* upper, int32_t* border, void* d_scratch, void* stream);
int sdfk_field_cell_counts(const float* d_field, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                           int64_t n2, float level, int64_t* counts, void* d_scratch, void* stream);
int sdfk_eval_grid_cell_counts(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                               const float* ax2, int64_t n2, float level, int64_t* counts, void* d_scratch, void* stream,
                               int mode);
int sdfk_label_field(const int32_t* d_labels, int64_t n, const unsigned char* keep, int64_t count, float inside,
                     float outside, float* d_out, void* stream);
int sdfk_label_moments(int64_t n0, int64_t n1, int64_t n2, const int32_t* d_labels, int64_t count, uint64_t* sums,
                       void* d_scratch, void* stream);

/* ---- layer graphs: the components of every layer of a plane stack and their links (aegolius_amd.layers;
 * csrc/sdfk_layers.inc) --------------------------------------------------------------------------------------------------
 * Grid: the three strictly increasing HOST tables heights (layers >= 2), u (nu >= 2), v (nv >= 2); the layer is the
 * slowest axis, flat index p = (l nu + i) nv + j; at most 2^31 - 1 points. Inside as in the topology block. Only the inside
 * points are labelled, and two points are joined only when they are neighbours within one layer (SDFK_CONNECT_FACES: 4,
 * SDFK_CONNECT_FULL: 8). Names (`first`, the smallest flat index) and ids (ascending `first`) as in the topology block, so
 * ids ascend with the layer. d_labels: layers nu nv int32, DEVICE, -1 off the inside.
 * sdfk_field_layer_label / sdfk_eval_grid_layer_label make the inside bits as sdfk_field_label / sdfk_eval_grid_label do
 * and label them with the passes of the topology block, the merge pass restricted to the backward row of the same layer;
 * sdfk_layer_label_bits labels the inside bits a previous topology or layer call left in the scratch. *count = K.
 * sdfk_layer_label_finish: the K records as sdfk_label_finish writes them (D = 3: lower[3 k] == upper[3 k] == the layer),
 * but border[k] = 1 only when a point of the component has i = 0, i = nu - 1, j = 0 or j = nv - 1: the first and the last
 * layer are no border. sdfk_label_finish refuses a layer labelling, and this call any other.
 * Links. overlap(c, q), c in layer l >= 1 and q in layer l - 1, is the number of columns (i, j) that carry c in layer l and
 * q in layer l - 1. A stretch is a maximal run of such columns within one grid row and one 32-point word of the bit string;
 * child and parent are constant in it. sdfk_layer_links, after a layer labelling with the same d_labels and scratch, counts
 * the stretches (*candidates = M) and writes supported[K] (HOST, int64): the sum of overlap(c, .), the points of c with an
 * inside point directly beneath; 0 in layer 0. sdfk_layer_links_finish writes the M candidates in word order, which does
 * not depend on scheduling: keys[M] (HOST, int64) = child << 32 | parent and lengths[M] (HOST, int32). A pair may come more
 * than once: overlap(c, q) is the sum of the lengths of its candidates, and the link list is the sorted unique keys — the
 * caller's reduction (layers.combine). 64-bit integer adds only. They allocate 8 bytes per component and 12 bytes per
 * candidate while they run.
 * d_scratch: sdfk_label_scratch(layers, nu, nv) bytes — the link pass needs nothing more: its per-tile counts and per-word
 * prefixes (1/8 byte per point) use regions of that layout the labelling leaves alone. pass_ms as in the topology block.
 * Return codes, refusals and the synchronous contract are those of the topology block: -7 when an iteration cap was
 * reached, or when sdfk_layer_links met a label that is no id below count; -1 and no launch also for nv = 1 (a 2-D grid),
 * a scratch that does not hold a layer labelling of that grid and count, or (finish) a link count of that size. Programs
 * with auxiliary fields (staged) are refused. */
int sdfk_field_layer_label(const float* d_field, const float* heights, int64_t layers, const float* u, int64_t nu,
                           const float* v, int64_t nv, float level, int connectivity, int32_t* d_labels, int64_t* count,
                           void* d_scratch, float* pass_ms, void* stream);
int sdfk_eval_grid_layer_label(sdfk_program* prog, const float* heights, int64_t layers, const float* u, int64_t nu,
                               const float* v, int64_t nv, float level, int connectivity, int32_t* d_labels, int64_t* count,
                               void* d_scratch, float* pass_ms, void* stream, int mode);
int sdfk_layer_label_bits(int64_t layers, int64_t nu, int64_t nv, int connectivity, int32_t* d_labels, int64_t* count,
                          void* d_scratch, float* pass_ms, void* stream);
int sdfk_layer_label_finish(int64_t layers, int64_t nu, int64_t nv, int64_t count, const int32_t* d_labels, int64_t* first,
                            int64_t* sizes, int32_t* lower, int32_t* upper, int32_t* border, void* d_scratch, void* stream);
int sdfk_layer_links(int64_t layers, int64_t nu, int64_t nv, int64_t count, const int32_t* d_labels, int64_t* candidates,
                     int64_t* supported, void* d_scratch, void* stream);
int sdfk_layer_links_finish(int64_t layers, int64_t nu, int64_t nv, int64_t count, const int32_t* d_labels, int64_t candidates,
                            int64_t* keys, int32_t* lengths, void* d_scratch, void* stream);

/* ---- sphere tracing ----------------------------------------------------------------------------
 * First hit of rays with the surface of the program's field, which must be a distance bound: |f(p) - f(q)| <=
 * L |p - q| with a finite L the caller knows (aegolius_amd._lower tracks it per program). Per ray, in fp32:
 *     t = t_min
 *     repeat at most max_steps times:
 *         f = field(o + t d);  thr = max(eps, cone * t)
 *         if f <= thr: status 1 (hit), stop
 *         t = t + f * inv_lipschitz;  steps += 1
 *         if t > t_max: status 0 (miss), stop
 *     otherwise: status 2 (step limit)
 * Outputs, one entry per ray: d_t (fp32, the parameter the ray stopped at), d_status (1 byte), d_steps (int32, the
 * advances made: 0 for a ray that starts within thr of the solid) and, unless d_normals is NULL, the unit normal at
 * the hit as three rows of normal_stride floats: the four-point tetrahedron difference of the field with the
 * half-width h = max(thr, 2^-16 * max(|x|, |y|, |z|)) of the hit point, the zero vector for rays that did not hit.
 * Directions must be unit vectors (not checked on the device). Asynchronous on `stream`. `mode` selects the kernel as
 * for sdfk_eval_device: the interpreter kernel and the specialised ones (SDFK_FLAVOUR_RAYS) give the same bits. A long
 * hard union (chain mode) is traced by a kernel that culls its members per wave — a survivor list in LDS for the
 * sphere around the points the wave evaluates next — under SDFK_MODE_SPECIALIZED and SDFK_MODE_AUTO, and by the plain
 * kernel, every member at every step, under SDFK_MODE_NOCULL; for every other program the two are the same kernel; programs beyond the interpreter's register
 * file run on the specialised kernel only. Arguments are validated on the host — t_max < t_min, max_steps <= 0, a
 * non-finite or non-positive inv_lipschitz, negative eps / cone return -1 and launch nothing. */
/* 0: the program can be traced; 1: it reads an auxiliary field (V_FIELD: staged evaluation, defined on a grid only),
 * *first_bad_op (nullable) = that instruction. */
int sdfk_program_rays_check(sdfk_program* prog, int* first_bad_op);
/* n rays from two (3, n) device arrays (row r of the origins at d_origins + r * origin_stride, likewise directions). */
int sdfk_trace_rays_device(sdfk_program* prog, const float* d_origins, int64_t origin_stride, const float* d_directions,
                           int64_t direction_stride, int64_t n, float t_min, float t_max, float eps, float cone,
                           float inv_lipschitz, int max_steps, float* d_t, unsigned char* d_status, int* d_steps,
                           float* d_normals, int64_t normal_stride, void* stream, int mode);
/* width x height rays generated in the kernel from `camera`, 12 host floats {eye, fwd, du, dv}: for pixel (ix, iy), row
 * 0 at the top, a = (2 ix + 1) / width - 1 and b = 1 - (2 iy + 1) / height;
 *     perspective : o = eye,                d = normalised(fwd + a du + b dv)
 *     orthographic: o = eye + a du + b dv,  d = fwd
 * (fwd a unit vector). Outputs in row-major pixel order (index iy * width + ix); every wave traces one tile of 8 x 8
 * pixels. */
int sdfk_trace_camera_device(sdfk_program* prog, const float* camera, int width, int height, int orthographic, float t_min,
                             float t_max, float eps, float cone, float inv_lipschitz, int max_steps, float* d_t,
                             unsigned char* d_status, int* d_steps, float* d_normals, int64_t normal_stride, void* stream,
                             int mode);

/* ---- spans: every crossing of a ray with the solid, and its chord ---------------------------------------------------
 * The march of sdfk_trace_rays_device does not stop at the surface: it records every change of sign of the field along
 * the ray and adds up the length inside the solid { f <= 0 }. The field must be a distance bound as above. Per ray, in fp32:
 *     t = t_min; count = 0; chord = 0
 *     repeat at most max_steps times (evaluation e = 0, 1, ...):
 *         f = field(o + t d);  inside = (f <= 0)
 *         if e == 0: was = inside0 = inside; t_in = t_min                  (starting inside is not a crossing)
 *         else if inside != was:
 *             tc = t_prev + (t - t_prev) * |f_prev| / (|f_prev| + |f|)     (secant, one fmaf)
 *             if count < max_crossings: crossings[count] = tc
 *             count += 1;  if inside: t_in = tc  else: chord += tc - t_in;  was = inside
 *         thr = max(eps, cone * t);  t_prev = t;  f_prev = f
 *         t_next = t + max(|f| * inv_lipschitz, thr);  steps += 1
 *         if not (t_next > t): status 2 (limit), stop                      (no progress in fp32)
 *         t = t_next
 *         if t > t_max: if was: chord += t_max - t_in;  status 0 (complete), stop
 *     otherwise: status 2 (limit)
 *     status 2, either way: if was: chord += t_prev - t_in                 (t_prev: the last evaluated parameter)
 * A step of |f| / L cannot cross the surface, so every crossing lies inside a floor step of length thr: it is bracketed
 * within thr, and only features thinner than thr along the ray can be missed, as a pair of crossings. eps must be large
 * enough for t + eps > t in fp32 over [t_min, t_max] (2^-20 max(|t_min|, |t_max|) is), or rays end with status 2.
 * Outputs, one entry per ray: d_chord (fp32), d_count (int32: all crossings, also those beyond max_crossings), d_status
 * (1 byte: 0 or 2, plus 4 when the ray is inside the solid at t_min), d_steps (int32: evaluations made) and, unless
 * d_crossings is NULL or max_crossings is 0, the first max_crossings crossing parameters as max_crossings rows of
 * crossing_stride floats: crossing k of ray i at d_crossings[k * crossing_stride + i]. Rows from `count` on are NOT
 * written: the caller initialises the array (NaN). Asynchronous on `stream`. `mode` selects the kernel exactly as for
 * sdfk_trace_rays_device (SDFK_FLAVOUR_SPANS; interpreter and specialised kernels give the same bits; long chains are
 * culled per wave except under SDFK_MODE_NOCULL, same bits). Programs with auxiliary fields are refused
 * (sdfk_program_rays_check). Validated on the host, -1 and no launch: what sdfk_trace_rays_device refuses, a NULL
 * d_chord / d_count / d_status / d_steps, max_crossings outside 0 ... 32, n < 0, crossing_stride < the ray count. */
int sdfk_span_rays_device(sdfk_program* prog, const float* d_origins, int64_t origin_stride, const float* d_directions,
                          int64_t direction_stride, int64_t n, float t_min, float t_max, float eps, float cone,
                          float inv_lipschitz, int max_steps, float* d_chord, int* d_count, unsigned char* d_status,
                          int* d_steps, float* d_crossings, int64_t crossing_stride, int max_crossings, void* stream, int mode);
/* width x height rays generated in the kernel from `camera` as by sdfk_trace_camera_device; outputs in row-major pixel
 * order, crossing k of pixel (ix, iy) at d_crossings[k * crossing_stride + iy * width + ix]; one tile of 8 x 8 pixels per wave. */
int sdfk_span_camera_device(sdfk_program* prog, const float* camera, int width, int height, int orthographic, float t_min,
                            float t_max, float eps, float cone, float inv_lipschitz, int max_steps, float* d_chord,
                            int* d_count, unsigned char* d_status, int* d_steps, float* d_crossings, int64_t crossing_stride,
                            int max_crossings, void* stream, int mode);

/* ---- secondary rays: what a surface point sees (csrc/sdfk_raydev.h: sdfk_trace_visibility, sdfk_trace_occlusion) ------
 * Visibility: how much of the segment [t_min, t_end] of a ray is free of the solid. Per ray i, in fp32:
 *     t = t_min; vis = 1; t_end = d_limits ? min(t_max, d_limits[i]) : t_max
 *     repeat at most max_steps times:
 *         f = field(o + t d);  thr = max(eps, cone * t)
 *         if f <= thr: vis = 0; status 1 (blocked), stop
 *         if softness > 0: vis = min(vis, softness * (f * inv_lipschitz) / t)       (t = 0: +inf, since f > 0)
 *         t = fmaf(f, inv_lipschitz, t);  steps += 1
 *         if t > t_end: status 0 (clear), stop
 *     otherwise: status 2 (step limit; vis is what was seen so far)
 * The advance and the two tests are those of sdfk_trace_rays_device: with d_limits NULL, d_status and d_steps are the
 * bytes that call writes, whatever the softness. softness = 0 is the hard test (vis is 0 or 1); with softness = k a ray
 * that passes the solid at a distance below t / k sees less than 1 (a light of angular radius about 1 / k). t_min >= 0,
 * so that vis lies in [0, 1]. d_limits (nullable): n floats, the end of every ray — the distance to a point light.
 * Outputs, one entry per ray: d_vis (fp32), d_status (1 byte), d_steps (int32). Asynchronous on `stream`; `mode` as for
 * sdfk_trace_rays_device (SDFK_FLAVOUR_SECONDARY; interpreter and specialised kernels give the same bits; long chains
 * are culled per wave except under SDFK_MODE_NOCULL, same bits). Validated on the host, -1 and no launch: what
 * sdfk_trace_rays_device refuses, t_min < 0, a negative or non-finite softness, a NULL d_vis / d_status / d_steps. */
int sdfk_visibility_rays_device(sdfk_program* prog, const float* d_origins, int64_t origin_stride, const float* d_directions,
                                int64_t direction_stride, int64_t n, float t_min, float t_max, float eps, float cone,
                                float inv_lipschitz, int max_steps, float softness, const float* d_limits, float* d_vis,
                                unsigned char* d_status, int* d_steps, void* stream, int mode);
/* Ambient occlusion of n points with unit normals (two (3, n) device arrays, rows strided as above). Per point, in fp32:
 *     occ = 0
 *     for i = 1 .. samples:  h = radius * i * (1 / samples);  f = field(p + h n)
 *                            occ = fmaf(2^-i, max(0, h - f * inv_lipschitz), occ)
 *     ao = min(1, max(0, 1 - strength * occ * (1 / radius)))           (1 / samples, 1 / radius rounded to fp32 once)
 * 1 above a plane, smaller where the solid comes closer to the samples than the point's own surface. d_ao: n floats.
 * `stream` and `mode` as above. -1 and no launch: radius not finite or <= 0, samples outside 1 ... 16, strength negative
 * or not finite, a bad inv_lipschitz, a NULL d_ao, n < 0, a row stride below n. */
int sdfk_occlusion_rays_device(sdfk_program* prog, const float* d_points, int64_t point_stride, const float* d_normals,
                               int64_t normal_stride, int64_t n, float radius, int samples, float strength,
                               float inv_lipschitz, float* d_ao, void* stream, int mode);

/* ---- sub-voxel occupancy (aegolius_amd.occupancy; csrc/sdfk_occupancy.inc, csrc/sdfk_occdev.h) ---------------------
 * Per cell of the grid of the axis tables (flat index (i0 n1 + i1) n2 + i2), the fraction of its K = k0 k1 k2 sub-sample
 * points (sub0[i0 k0 + j0], sub1[i1 k1 + j1], sub2[i2 k2 + j2]) whose field value is <= level (NaN: outside); k_a =
 * samples (1, 2, 4 or 8) on an axis of more than one point and 1 on an axis of one point. d_fraction: n0 n1 n2 floats,
 * count / K, exact. All tables are HOST pointers: ax* the grid points (n_a floats, what sdfk_eval_grid takes), sub* the
 * sub-sample coordinates (n_a k_a floats), hw* per grid point an upper bound of its distance to its farthest sub-sample
 * along that axis (n_a floats). `lipschitz`: |f(p) - f(q)| <= L |p - q|. A cell with
 *     |f(c) - level| > 1.0001 L rho + L cmag + 1e-6 (1 + |f(c)| + |level|),   rho = sqrt(hw0^2 + hw1^2 + hw2^2),
 *     cmag = 1e-6 (|cx| + |cy| + |cz| + rho)
 * (fp32; false if a side is NaN) is entirely in or out and gets 1.0 / 0.0 by its centre value, which the grid kernels of
 * sdfk_eval_grid compute; only the other cells ("near") are sampled. L = +infinity, or SDFK_MODE_NOCULL: no cell is
 * skipped and the centre values are not computed. Too small an L gives wrong fractions. The grid is processed in slabs of
 * whole rows of at most slab_cells cells (<= 0 or more than 2^30: 2^30); d_scratch: *_scratch bytes (8 per slab cell, 8
 * per 1024 slab cells and 32 KB), 256-byte aligned. *inside_samples = the sum of the counts (integers added on the
 * device and the host: exact, whatever the order), *near_cells = the cells that were sampled. pass_ms (nullable): 3 floats that receive device-event milliseconds
 * of the centre values, the classification and the sampling. `mode` as for sdfk_trace_rays_device: the interpreter sample
 * kernel and the specialised one (SDFK_FLAVOUR_OCCUPANCY) give the same bits. Programs with auxiliary fields are refused
 * (sdfk_program_rays_check). Synchronous: the stream is idle on return. */
size_t sdfk_eval_grid_occupancy_scratch(int64_t n0, int64_t n1, int64_t n2, int64_t slab_cells);
int sdfk_eval_grid_occupancy(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                             int64_t n2, const float* sub0, const float* sub1, const float* sub2, const float* hw0,
                             const float* hw1, const float* hw2, int samples, float level, float lipschitz, float* d_fraction,
                             void* d_scratch, int64_t slab_cells, int64_t* inside_samples, int64_t* near_cells, float* pass_ms,
                             void* stream, int mode);
/* d_out[r] = sum over i of d_field[r row_len + i] * weights[i] in float64, in a fixed order (weights: HOST, row_len
 * doubles; d_out: rows doubles, DEVICE). What the volume of the fractions is reduced with. Synchronous. */
int sdfk_field_row_sums(const float* d_field, int64_t rows, int64_t row_len, const double* weights, double* d_out, void* stream);

/* ---- mass properties (aegolius_amd.moments; csrc/sdfk_moments.inc, csrc/sdfk_momdev.h) -------------------------------
 * The integer moments of the solid on the sub-sample lattice of sdfk_eval_grid_occupancy — same tables, same "inside",
 * same far rule, same slabs, every argument up to `lipschitz` as there. Sub-sample j_a of grid point i_a has the odd
 * lattice coordinate u_a = 2 (i_a k_a + j_a) + 1; over all inside sub-samples,
 *     M = (N, U0, U1, U2, U00, U01, U02, U11, U12, U22) = the sums of 1, u_a, u_a u_b   (an axis of one point: u = 1).
 * moments_out: HOST, 20 uint64 — M[t] = moments_out[2 t] + 2^64 moments_out[2 t + 1], exact, whatever the order of the
 * waves: the device keeps 64-bit partial sums per wave, the host adds them in 128 bits. Far cells on the inside enter
 * in closed form (no field evaluation), near cells are sampled, one sub-sample per lane; *near_cells = the cells that
 * were sampled, the number sdfk_eval_grid_occupancy reports. No per-cell output is made. d_scratch: scratch_bytes >=
 * *_scratch bytes (8 per slab cell, 8 per 1024 slab cells and the partials: at most 11 MB), 256-byte aligned. pass_ms
 * (nullable): 3 floats that receive device-event milliseconds of the centre values, the far pass (classification and
 * the far cells' sums) and the sampling. `mode` as for sdfk_eval_grid_occupancy (SDFK_FLAVOUR_MOMENTS). -1 and no
 * launch: a NULL pointer, samples, a NaN level, a bad bound, an unknown mode, too small a scratch buffer, an axis of 2^31
 * sub-samples or more; -2 and no launch: a grid so long that a 64-bit partial could wrap. Programs with auxiliary fields
 * are refused (sdfk_program_rays_check). Synchronous: the stream is idle on return. */
size_t sdfk_eval_grid_moments_scratch(int64_t n0, int64_t n1, int64_t n2, int64_t slab_cells);
int sdfk_eval_grid_moments(sdfk_program* prog, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                           int64_t n2, const float* sub0, const float* sub1, const float* sub2, const float* hw0,
                           const float* hw1, const float* hw2, int samples, float level, float lipschitz, void* d_scratch,
                           size_t scratch_bytes, int64_t slab_cells, uint64_t* moments_out, int64_t* near_cells,
                           float* pass_ms, void* stream, int mode);

/* ---- redistancing (aegolius_amd.redistance; csrc/sdfk_redistance.inc) ------------------------------------------------
 * d_out[p] = the signed Euclidean distance of grid point p (flat index (i0 n1 + i1) n2 + i2) to the level set of the
 * field, the level set being the crossing vertices of sdfk_field_isosurface / sdfk_field_contour2d: negative where
 * f <= level, NaN counting as outside. The definition, float32 operation by operation, is the module text of
 * aegolius_amd/redistance.py; the result is the brute-force minimum over all seeds of that expression, bit for bit. ax*:
 * HOST tables, finite and strictly increasing, n0 and n1 >= 2; n2 = 1 is a 2-D grid (ax2 is then not read). band <= 0:
 * none; else finite, the distance is cut at it: min(D, band). near: 0 = the distance to the seeds alone, 1 = the points
 * at the ends of crossing edges take min(D, |f - level| / |grad f|) in addition. d_field (n0 n1 n2 floats) is only
 * read and must not be d_out. d_scratch: *_scratch bytes = 2 n0 n1 n2 floats, nothing is written beyond them. *seeds =
 * the number of seeds (crossing edges). pass_ms (nullable): SDFK_REDISTANCE_PASSES floats that receive device-event
 * milliseconds, 3-D: the passes x, xy, y, yx (merged), z of the merged, z, zx, zxy, then the finish; 2-D: x, xy, y, yx,
 * finish, the rest 0. Synchronous: the stream is idle on return. */
#define SDFK_REDISTANCE_PASSES 9
size_t sdfk_field_redistance_scratch(int64_t n0, int64_t n1, int64_t n2);
int sdfk_field_redistance(const float* d_field, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                          int64_t n2, float level, float band, int near, float* d_out, void* d_scratch, int64_t* seeds,
                          float* pass_ms, void* stream);

/* ---- interval enclosures (aegolius_amd.enclosure; csrc/sdfk_enclosure.inc, csrc/sdfk_boxdev.h) ------------------------
 * An enclosure of a program over an axis-aligned box B is a pair [lo, hi] with lo <= f(p) <= hi for every fp32 point p of
 * B, f being the fp32 field the evaluation kernels compute; an end is never NaN (a rule that cannot bound gives -inf /
 * +inf). The rules, their padding (sdfk_box_pad_ulps() ulps of the largest magnitude a rule handles) and the contract are
 * in csrc/sdfk_boxdev.h and DESIGN.md 4.17. d_factors: one float per instruction, DEVICE: the Lipschitz factor of a
 * coordinate operation (+inf: none), the Lipschitz constant of a primitive, anything for value operations. */
int sdfk_box_pad_ulps(void);
/* 1 if the opcode has a box rule. */
int sdfk_box_has_rule(int op);
/* 0: every instruction has a box rule and the program fits the kernel's 16 coordinate / 8 value registers; 1: an
 * instruction without a rule, *first_bad_op (nullable) = its index; 2: the register files are exceeded. */
int sdfk_program_box_check(sdfk_program* prog, int* first_bad_op);
/* n boxes: row r of the lower ends at d_lo + r * stride, r = 0, 1, 2 = x, y, z, likewise d_hi (fp32, lo <= hi, finite: not
 * checked on the device). d_out_lo / d_out_hi: n floats each. One box per lane, every instruction evaluated. Asynchronous
 * on `stream`. */
int sdfk_enclose_boxes_device(sdfk_program* prog, const float* d_lo, const float* d_hi, int64_t n, int64_t stride,
                              const float* d_factors, float* d_out_lo, float* d_out_hi, void* stream);
/* One refinement step of an octree (dims = 3) or quadtree (dims = 2: z = 0) over `domain` = {lo x, y, z, hi x, y, z}
 * (HOST doubles). d_keys: n box keys, level << 57 | ix << 38 | iy << 19 | iz with 0 <= i < 2^level, level <= 19. The box of
 * a key along an axis is [lo + (hi - lo) (i / 2^level), lo + (hi - lo) ((i + 1) / 2^level)] in float64 as written (the last
 * cell ends at hi itself), rounded outward to fp32. d_status[k] = -1 when the box is entirely inside (enclosure hi <=
 * level), +1 entirely outside (lo > level), 0 mixed (d_status may be NULL: the counts alone). The 8 (4) children of every mixed key are appended to d_children in
 * no particular order, never beyond `capacity` keys (capacity 0: nothing is written and d_children may be NULL);
 * *needed = the number of children there are, so a caller whose capacity was too small learns the size to ask for.
 * counts[3] = boxes inside, outside, mixed; hull[6] = minimum and maximum (ix, iy, iz) of the leaves that are not outside:
 * the inside boxes and, when no child list is kept (capacity 0: the last level), the mixed ones (0x7fffffff / -1 when
 * there are none). d_scratch: sdfk_enclose_octree_scratch() bytes. Synchronous. */
size_t sdfk_enclose_octree_scratch(void);
int sdfk_enclose_octree_device(sdfk_program* prog, const uint64_t* d_keys, int64_t n, const double* domain, int dims,
                               float level, const float* d_factors, signed char* d_status, uint64_t* d_children,
                               int64_t capacity, int64_t* needed, int64_t* counts, int* hull, void* d_scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFK_H */
