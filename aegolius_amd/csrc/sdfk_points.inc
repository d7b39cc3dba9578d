// Points.to_image (reference cores/geom.py, Points.to_image), included from sdfk.hip.
//
// The reference bins the cloud with numpy.histogramdd onto a float64 (rx, ry, rz) grid, keeps "count > 0" and then
// extends the occupied region plane by plane. Here the grid is one byte per voxel in HBM:
//   bin     one point per lane: per axis a float64 binary search of the edge table with searchsorted(side='right')
//           semantics, a point on the last edge moved into the last bin, indices 0 and n + 1 dropped (outliers, and
//           NaN, detected from its bits because the library is built with -fno-honor-nans). A kept point writes 1 to
//           its voxel: the write is idempotent, so concurrent writers need no atomics.
//   extent  one pass over the grid: a wave per z row, an LDS byte array for the block's z flags, three per-plane
//           "any" arrays (x, y, z) written with idempotent byte writes of 1.
//   fill    copies an occupied plane over a range of planes of one axis: whole contiguous slabs (x), rows (y), or a
//           byte broadcast along each z row (z). The source plane is never inside the written range.
//   widen   byte -> float64 (host result) or float32 (DeviceField).
// Voxel indices are 64-bit throughout: grids above 2^31 voxels work.

#define SDFK_PTS_BLOCK 256
#define SDFK_PTS_MAX_RZ 65536       // LDS z-flag array of the extent pass

// searchsorted(edges[0..m), v, side='right'): the number of edges <= v
static __device__ __forceinline__ long long pts_search_right(const double* __restrict__ e, long long m, double v) {
    long long lo = 0, hi = m;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (e[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// numpy.histogramdd's bin of v on one axis (n bins, n + 1 edges), or -1 for an outlier / NaN
static __device__ __forceinline__ long long pts_bin(const double* __restrict__ e, long long n, double v) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    if ((bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return -1;      // NaN: numpy sorts it past the end
    long long c = pts_search_right(e, n + 1, v);
    if (v == e[n]) c -= 1;                                                          // on the last edge: last bin
    return (c >= 1 && c <= n) ? c - 1 : -1;
}

__global__ __launch_bounds__(SDFK_PTS_BLOCK) void sdfk_points_bin_kernel(const double* __restrict__ cloud, long long n,
                                                                          long long row_stride,
                                                                          const double* __restrict__ edges, long long rx,
                                                                          long long ry, long long rz,
                                                                          unsigned char* __restrict__ grid) {
    const double* ex = edges;
    const double* ey = ex + rx + 1;
    const double* ez = ey + ry + 1;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const long long i = pts_bin(ex, rx, cloud[p]);
        const long long j = pts_bin(ey, ry, cloud[row_stride + p]);
        const long long k = pts_bin(ez, rz, cloud[2 * row_stride + p]);
        if (i >= 0 && j >= 0 && k >= 0) grid[(i * ry + j) * rz + k] = 1;
    }
}

// flags: rx bytes (x planes), then ry (y planes), then rz (z planes); zeroed by the caller's launch
__global__ __launch_bounds__(SDFK_PTS_BLOCK) void sdfk_points_extent_kernel(const unsigned char* __restrict__ grid,
                                                                             long long rx, long long ry, long long rz,
                                                                             unsigned char* __restrict__ flags) {
    extern __shared__ unsigned char zloc[];
    for (long long k = threadIdx.x; k < rz; k += blockDim.x) zloc[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const long long rows = rx * ry;
    for (long long r = (long long)blockIdx.x * waves + wave; r < rows; r += (long long)gridDim.x * waves) {
        const unsigned char* row = grid + r * rz;
        int any = 0;
        for (long long k = lane; k < rz; k += 64) {
            if (row[k]) {
                zloc[k] = 1;
                any = 1;
            }
        }
        if (__any(any) && lane == 0) {
            flags[r / ry] = 1;
            flags[rx + r % ry] = 1;
        }
    }
    __syncthreads();
    for (long long k = threadIdx.x; k < rz; k += blockDim.x)
        if (zloc[k]) flags[rx + ry + k] = 1;
}

// planes [lo, lo + len) of the middle axis of an (outer, na, inner) view take the contents of plane src: x (outer = 1,
// inner = ry rz) copies slabs, y (outer = rx, inner = rz) copies rows. One block per destination run.
__global__ __launch_bounds__(SDFK_PTS_BLOCK) void sdfk_points_fill_runs_kernel(unsigned char* __restrict__ grid,
                                                                                long long outer, long long na,
                                                                                long long inner, long long src, long long lo,
                                                                                long long len) {
    const long long runs = outer * len;
    for (long long r = blockIdx.x; r < runs; r += gridDim.x) {
        const long long o = r / len, c = lo + r % len;
        const unsigned char* s = grid + (o * na + src) * inner;
        unsigned char* d = grid + (o * na + c) * inner;
        for (long long t = threadIdx.x; t < inner; t += blockDim.x) d[t] = s[t];
    }
}

// z: in every row, bytes [lo, lo + len) take the value of byte src
__global__ __launch_bounds__(SDFK_PTS_BLOCK) void sdfk_points_fill_z_kernel(unsigned char* __restrict__ grid, long long rows,
                                                                             long long rz, long long src, long long lo,
                                                                             long long len) {
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        unsigned char* row = grid + r * rz;
        const unsigned char v = row[src];
        for (long long t = threadIdx.x; t < len; t += blockDim.x) row[lo + t] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(SDFK_PTS_BLOCK) void sdfk_points_widen_kernel(const unsigned char* __restrict__ grid, long long n,
                                                                            T* __restrict__ out) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x)
        out[p] = grid[p] ? (T)1 : (T)0;
}

static unsigned pts_blocks(long long work) {
    const long long b = (work + SDFK_PTS_BLOCK - 1) / SDFK_PTS_BLOCK;
    return (unsigned)std::max<long long>(1, std::min<long long>(b, 1 << 20));
}

static int pts_dims_ok(long long rx, long long ry, long long rz, const char* who) {
    if (rx < 1 || ry < 1 || rz < 1) return fail(-1, std::string(who) + ": every resolution must be at least 1");
    if (rx > (1ll << 40) / ry / rz) return fail(-1, std::string(who) + ": grid too large");
    return 0;
}

extern "C" int sdfk_points_bin(const double* d_cloud, int64_t n, int64_t row_stride, const double* d_edges, int64_t rx,
                               int64_t ry, int64_t rz, unsigned char* d_grid, void* stream_) {
    int rc = pts_dims_ok(rx, ry, rz, "sdfk_points_bin");
    if (rc) return rc;
    if (!d_edges || !d_grid || (n > 0 && !d_cloud)) return fail(-1, "sdfk_points_bin: null pointer");
    if (n < 0 || row_stride < n) return fail(-1, "sdfk_points_bin: bad point count or row stride");
    hipStream_t stream = (hipStream_t)stream_;
    hipError_t e = hipMemsetAsync(d_grid, 0, (size_t)(rx * ry * rz), stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_points_bin: ") + hipGetErrorString(e));
    if (n > 0) {
        hipLaunchKernelGGL(sdfk_points_bin_kernel, dim3(pts_blocks(n)), dim3(SDFK_PTS_BLOCK), 0, stream, d_cloud,
                           (long long)n, (long long)row_stride, d_edges, (long long)rx, (long long)ry, (long long)rz, d_grid);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(-6, std::string("sdfk_points_bin: ") + hipGetErrorString(e));
    }
    return 0;
}

extern "C" int sdfk_points_extent(const unsigned char* d_grid, int64_t rx, int64_t ry, int64_t rz, unsigned char* d_flags,
                                  void* stream_) {
    int rc = pts_dims_ok(rx, ry, rz, "sdfk_points_extent");
    if (rc) return rc;
    if (!d_grid || !d_flags) return fail(-1, "sdfk_points_extent: null pointer");
    if (rz > SDFK_PTS_MAX_RZ) return fail(-1, "sdfk_points_extent: z resolution beyond 65536");
    hipStream_t stream = (hipStream_t)stream_;
    hipError_t e = hipMemsetAsync(d_flags, 0, (size_t)(rx + ry + rz), stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_points_extent: ") + hipGetErrorString(e));
    const long long rows = rx * ry, waves = SDFK_PTS_BLOCK / 64;
    const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((rows + waves - 1) / waves, 2048));
    hipLaunchKernelGGL(sdfk_points_extent_kernel, dim3(blocks), dim3(SDFK_PTS_BLOCK), (size_t)rz, stream, d_grid,
                       (long long)rx, (long long)ry, (long long)rz, d_flags);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(-6, std::string("sdfk_points_extent: ") + hipGetErrorString(e));
    return 0;
}

// axis 0 / 1 / 2 = x / y / z: planes [lo, hi) of that axis become copies of plane src (src outside [lo, hi))
extern "C" int sdfk_points_fill(unsigned char* d_grid, int64_t rx, int64_t ry, int64_t rz, int axis, int64_t src, int64_t lo,
                                int64_t hi, void* stream_) {
    int rc = pts_dims_ok(rx, ry, rz, "sdfk_points_fill");
    if (rc) return rc;
    if (!d_grid) return fail(-1, "sdfk_points_fill: null grid");
    if (axis < 0 || axis > 2) return fail(-1, "sdfk_points_fill: axis must be 0, 1 or 2");
    const long long na = axis == 0 ? rx : axis == 1 ? ry : rz;
    if (!(0 <= lo && lo <= hi && hi <= na && 0 <= src && src < na && (src < lo || src >= hi)))
        return fail(-1, "sdfk_points_fill: bad plane range");
    if (hi == lo) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const long long len = hi - lo;
    if (axis == 2) {
        const long long rows = rx * ry;
        hipLaunchKernelGGL(sdfk_points_fill_z_kernel, dim3((unsigned)std::min<long long>(rows, 1 << 20)),
                           dim3(SDFK_PTS_BLOCK), 0, stream, d_grid, rows, (long long)rz, (long long)src, (long long)lo, len);
    } else {
        const long long outer = axis == 0 ? 1 : rx, inner = axis == 0 ? ry * rz : rz;
        hipLaunchKernelGGL(sdfk_points_fill_runs_kernel, dim3((unsigned)std::min<long long>(outer * len, 1 << 20)),
                           dim3(SDFK_PTS_BLOCK), 0, stream, d_grid, outer, na, inner, (long long)src, (long long)lo, len);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-6, std::string("sdfk_points_fill: ") + hipGetErrorString(e));
    return 0;
}

// kind 0: float64 out (8 bytes per voxel), kind 1: float32 out
extern "C" int sdfk_points_widen(const unsigned char* d_grid, int64_t n, int kind, void* d_out, void* stream_) {
    if (!d_grid || !d_out) return fail(-1, "sdfk_points_widen: null pointer");
    if (n < 0 || (kind != 0 && kind != 1)) return fail(-1, "sdfk_points_widen: bad size or kind");
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    if (kind == 0)
        hipLaunchKernelGGL(sdfk_points_widen_kernel<double>, dim3(pts_blocks(n)), dim3(SDFK_PTS_BLOCK), 0, stream, d_grid,
                           (long long)n, static_cast<double*>(d_out));
    else
        hipLaunchKernelGGL(sdfk_points_widen_kernel<float>, dim3(pts_blocks(n)), dim3(SDFK_PTS_BLOCK), 0, stream, d_grid,
                           (long long)n, static_cast<float*>(d_out));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-6, std::string("sdfk_points_widen: ") + hipGetErrorString(e));
    return 0;
}
