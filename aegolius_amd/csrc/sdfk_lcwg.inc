// Liquid-crystal waveguide (LCWG) director fields (reference cores/vector_functions_special.py), included from sdfk.hip.
//
// Two pieces:
//   crossings  compute_crossings_2d (:14-36) on grid plane k = 0 of a device field (or of pp computed from two fields):
//              plane minimum, one wave per row for the parity scan along j (ballot + prefix popcount), then the two 5x5
//              reflect-mode box averages of conv_averaging counted in integers (the average is c / 625, so
//              average >= 0.5 is c >= 313) and written as int8 +-1.
//   fields     lcwg1_2d / lcwg1_p1 / lcwg1_m1 (:127-251) in ONE pass: every thread owns a (j, k) column of the grid and
//              walks a few planes along i, carrying the stencil values (uu, or pp = |(2uu/w, ww/d)|) of planes i - 1,
//              i, i + 1 in registers; the four in-plane neighbours are recomputed. numpy.gradient, the normalisations,
//              the two Rodrigues rotations and the final normalisation follow in registers; three fp32 rows out.
//              The lcwg1_*_old forms are a pointwise kernel of their own.
// Arithmetic is float64 from the fp32 inputs, in numpy's order (build flags: -ffp-contract=off). That makes the fused
// kernel VALU-bound (DESIGN.md 4.8.1), and it is what decides the sign of the output where the reference's rotation
// angles sit exactly on pi/2 or 3pi/2: there cos() of the float64 angle is +6.1e-17 / -1.8e-16 while fp32 gets the
// opposite signs, and at the points where the gradient has no xy part (e1 = e2 = 0) the output is +-vec by that sign
// alone. The plane of the crossings is the reference's bit for bit on fp32-representable inputs.

#define SDFK_LCWG_SEG 4            // planes a thread walks along axis 0

static __device__ __forceinline__ double lcwg_value(const float* __restrict__ uu, const float* __restrict__ ww, long long p,
                                                    double w, double d) {
    if (!ww) return (double)uu[p];
    const double a = 2.0 * (double)uu[p] / w, b = (double)ww[p] / d;     // numpy.linalg.norm([2uu/w, ww/d], axis=0)
    return sqrt(a * a + b * b);
}

// numpy.isclose(v, m, rtol=1e-5, atol=thr)
static __device__ __forceinline__ bool lcwg_close(double v, double m, double thr) { return fabs(v - m) <= thr + 1e-5 * fabs(m); }

// scipy.ndimage "reflect" (d c b a | a b c d | d c b a), also for axes shorter than the kernel's half width
static __device__ __forceinline__ int lcwg_reflect(int x, int n) {
    const int period = 2 * n;
    x %= period;
    if (x < 0) x += period;
    return x >= n ? period - 1 - x : x;
}

__global__ __launch_bounds__(1024) void sdfk_lcwg_plane_min_kernel(const float* __restrict__ uu, const float* __restrict__ ww,
                                                                    long long rows, long long n2, double w, double d,
                                                                    double* __restrict__ out_min) {
    __shared__ double part[1024];
    double m = INFINITY;
    for (long long t = sdfk_tx(); t < rows; t += 1024) m = fmin(m, lcwg_value(uu, ww, t * n2, w, d));
    part[sdfk_tx()] = m;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)sdfk_tx() < s) part[sdfk_tx()] = fmin(part[sdfk_tx()], part[sdfk_tx() + s]);
        __syncthreads();
    }
    if (sdfk_tx() == 0) *out_min = part[0];
}

// one wave per row i of the (n0, n1) plane: c1[j] = close(j) & !close(j - 1) for j >= 1, parity of the running count
__global__ __launch_bounds__(256) void sdfk_lcwg_parity_kernel(const float* __restrict__ uu, const float* __restrict__ ww,
                                                                int n0, int n1, long long n2, double w, double d, double thr,
                                                                const double* __restrict__ d_min,
                                                                unsigned char* __restrict__ parity) {
    const int lane = sdfk_tx() & 63;
    const long long i = (long long)sdfk_bx() * 4 + (sdfk_tx() >> 6);
    if (i >= n0) return;
    const double m = *d_min;
    unsigned carry = 0;
    for (int j0 = 0; j0 < n1; j0 += 64) {
        const int j = j0 + lane;
        bool flag = false;
        if (j >= 1 && j < n1) {
            const long long row = i * n1;
            flag = lcwg_close(lcwg_value(uu, ww, (row + j) * n2, w, d), m, thr) &&
                   !lcwg_close(lcwg_value(uu, ww, (row + j - 1) * n2, w, d), m, thr);
        }
        const unsigned long long mask = __ballot(flag);
        const unsigned upto = (unsigned)__popcll(mask & ((2ull << lane) - 1ull));   // lane 63: 2 << 63 wraps to 0 -> all bits
        if (j < n1) parity[i * n1 + j] = (unsigned char)((carry + upto) & 1u);
        carry = (carry + (unsigned)__popcll(mask)) & 1u;
    }
}

// one 5x5 reflect-mode box sum of the (n0, n1) plane; FINAL: the second pass, +-1 by c >= 313 (c / 625 >= 0.5)
template <bool FINAL>
__global__ __launch_bounds__(256) void sdfk_lcwg_box5_kernel(const unsigned char* __restrict__ in, int n0, int n1,
                                                              unsigned char* __restrict__ mid, signed char* __restrict__ sign) {
    const long long t = (long long)sdfk_bx() * 256 + sdfk_tx();
    if (t >= (long long)n0 * n1) return;
    const int i = (int)(t / n1), j = (int)(t - (long long)i * n1);
    int c = 0;
    for (int di = -2; di <= 2; ++di) {
        const long long row = (long long)lcwg_reflect(i + di, n0) * n1;
        for (int dj = -2; dj <= 2; ++dj) c += in[row + lcwg_reflect(j + dj, n1)];
    }
    if (FINAL)
        sign[t] = c >= 313 ? 1 : -1;
    else
        mid[t] = (unsigned char)c;
}

extern "C" int sdfk_field_crossings_2d(const float* d_uu, const float* d_ww, int64_t n0, int64_t n1, int64_t n2, double w,
                                       double d, double thr, signed char* d_sign, void* stream_) {
    GridDims g;
    if (!d_uu || !d_sign) return fail(-1, "sdfk_field_crossings_2d: null pointer");
    int rc = grid_dims_ok(n0, n1, n2, &g, "sdfk_field_crossings_2d");
    if (rc) return rc;
    if (d_ww && (w == 0.0 || d == 0.0)) return fail(-1, "sdfk_field_crossings_2d: w and d must not be 0");
    hipStream_t stream = (hipStream_t)stream_;
    const long long rows = (long long)n0 * n1;
    // work: the minimum (8 bytes, padded) and two byte planes
    char* work = nullptr;
    HIPCHK(hipMalloc((void**)&work, 16 + 2 * rows));
    double* d_min = reinterpret_cast<double*>(work);
    unsigned char* parity = reinterpret_cast<unsigned char*>(work + 16);
    unsigned char* mid = parity + rows;
    hipLaunchKernelGGL(sdfk_lcwg_plane_min_kernel, dim3(1), dim3(1024), 0, stream, d_uu, d_ww, rows, (long long)n2, w, d, d_min);
    hipLaunchKernelGGL(sdfk_lcwg_parity_kernel, dim3((unsigned)((n0 + 3) / 4)), dim3(256), 0, stream, d_uu, d_ww, g.n0, g.n1,
                       (long long)n2, w, d, thr, d_min, parity);
    hipLaunchKernelGGL(sdfk_lcwg_box5_kernel<false>, dim3(blocks256(rows)), dim3(256), 0, stream, parity, g.n0, g.n1, mid,
                       nullptr);
    hipLaunchKernelGGL(sdfk_lcwg_box5_kernel<true>, dim3(blocks256(rows)), dim3(256), 0, stream, mid, g.n0, g.n1, nullptr,
                       d_sign);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(work);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_field_crossings_2d: ") + hipGetErrorString(e));
    return 0;
}

// numpy.gradient along one axis, unit spacing, edge_order 1 (the axis has >= 2 points)
static __device__ __forceinline__ double lcwg_diff(double lo, double c, double hi, int idx, int n) {
    if (idx == 0) return hi - c;
    if (idx == n - 1) return c - lo;
    return (hi - lo) / 2.0;
}

// batch_normalize (cores/vector_modification_functions.py:14-20): zero vectors stay zero
static __device__ __forceinline__ void lcwg_normalize(double& x, double& y, double& z) {
    const double m = sqrt(x * x + y * y + z * z);
    if (m != 0.0) {
        x = x / m;
        y = y / m;
        z = z / m;
    }
}

// rotate_vectors_axis (:106-119): v cos + sin (a x v) + ((1 - cos) a) (v . a)
static __device__ __forceinline__ void lcwg_rotate(double& x, double& y, double& z, double ax, double ay, double az, double angle) {
    const double sa = sin(angle), ca = cos(angle);
    const double cx = ay * z - az * y, cy = az * x - ax * z, cz = ax * y - ay * x;
    const double dot = x * ax + y * ay + z * az, omc = 1.0 - ca;
    const double ox = x * ca + sa * cx + omc * ax * dot;
    const double oy = y * ca + sa * cy + omc * ay * dot;
    const double oz = z * ca + sa * cz + omc * az * dot;
    x = ox;
    y = oy;
    z = oz;
}

// VARIANT 0: lcwg1_2d (value = uu); 1: lcwg1_p1, 2: lcwg1_m1 (value = pp). sign_kind 0: the number `sign_value`,
// 1: int8 plane indexed by p / n2, 2: one fp32 number per point.
template <int VARIANT>
__global__ __launch_bounds__(256) void sdfk_lcwg_kernel(const float* __restrict__ uu, const float* __restrict__ ww, GridDims g,
                                                         double w, double d, int sign_kind, double sign_value,
                                                         const void* __restrict__ sign, float* __restrict__ out,
                                                         long long stride) {
    const long long plane = (long long)g.n1 * g.n2;
    const long long q = (long long)sdfk_bx() * 256 + sdfk_tx();
    if (q >= plane) return;
    const int i0 = (int)blockIdx.y * SDFK_LCWG_SEG, i1 = min(i0 + SDFK_LCWG_SEG, g.n0);
    const int j = (int)(q / g.n2), k = (int)(q - (long long)j * g.n2);
    const float* vw = VARIANT ? ww : nullptr;
    long long p = (long long)i0 * plane + q;
    double behind = i0 > 0 ? lcwg_value(uu, vw, p - plane, w, d) : 0.0;
    double centre = lcwg_value(uu, vw, p, w, d);
    for (int i = i0; i < i1; ++i, p += plane) {
        const double ahead = i + 1 < g.n0 ? lcwg_value(uu, vw, p + plane, w, d) : 0.0;
        const double ylo = j > 0 ? lcwg_value(uu, vw, p - g.n2, w, d) : 0.0;
        const double yhi = j + 1 < g.n1 ? lcwg_value(uu, vw, p + g.n2, w, d) : 0.0;
        const double zlo = k > 0 ? lcwg_value(uu, vw, p - 1, w, d) : 0.0;
        const double zhi = k + 1 < g.n2 ? lcwg_value(uu, vw, p + 1, w, d) : 0.0;
        double vx = lcwg_diff(behind, centre, ahead, i, g.n0);
        double vy = lcwg_diff(ylo, centre, yhi, j, g.n1);
        double vz = lcwg_diff(zlo, centre, zhi, k, g.n2);
        double s = sign_value;
        if (sign_kind == 1) s = (double)static_cast<const signed char*>(sign)[(long long)i * g.n1 + j];   // plane (i, j)
        else if (sign_kind == 2) s = (double)static_cast<const float*>(sign)[p];
        double ox, oy, oz;
        if (VARIANT == 0) {
            const double qq = fmin(fmax(2.0 * centre / w, 0.0), 1.0);
            const double phis = s * (qq * M_PI + M_PI / 2);
            const double sap = sin(phis), cap = cos(phis);
            ox = vx * cap - vy * sap;
            oy = vx * sap + vy * cap;
            oz = vz;
        } else {
            lcwg_normalize(vx, vy, vz);
            double e1x = -vy, e1y = vx, e1z = 0.0;
            lcwg_normalize(e1x, e1y, e1z);
            const double e2x = vy * e1z - vz * e1y, e2y = vz * e1x - vx * e1z, e2z = vx * e1y - vy * e1x;   // vec x e1
            const double qq = fmin(fmax(centre, 0.0), 1.0);
            const double phis = s * (qq * M_PI + M_PI / 2);
            ox = vx;
            oy = vy;
            oz = vz;
            lcwg_rotate(ox, oy, oz, e2x, e2y, e2z, phis);
            const double u = (double)uu[p], v = (double)ww[p];
            double alpha = atan2(2.0 * v / (d * d), 8.0 * u / (w * w));
            if (VARIANT == 2) alpha = -alpha;
            lcwg_rotate(ox, oy, oz, e1x, e1y, e1z, -2.0 * alpha);
        }
        lcwg_normalize(ox, oy, oz);
        out[p] = (float)ox;
        out[stride + p] = (float)oy;
        out[2 * stride + p] = (float)oz;
        behind = centre;
        centre = ahead;
    }
}

extern "C" int sdfk_lcwg_eval(int variant, const float* d_uu, const float* d_ww, int64_t n0, int64_t n1, int64_t n2, double w,
                              double d, int sign_kind, double sign_value, const void* d_sign, float* d_vec, int64_t row_stride,
                              void* stream_) {
    GridDims g;
    if (variant < 0 || variant > 2) return fail(-1, "sdfk_lcwg_eval: variant must be 0 (2D), 1 (p1) or 2 (m1)");
    if (!d_uu || !d_vec || (variant && !d_ww)) return fail(-1, "sdfk_lcwg_eval: null pointer");
    if (sign_kind < 0 || sign_kind > 2 || (sign_kind && !d_sign)) return fail(-1, "sdfk_lcwg_eval: bad sign operand");
    int rc = grid_dims_ok(n0, n1, n2, &g, "sdfk_lcwg_eval");
    if (rc) return rc;
    if (n0 < 2 || n1 < 2 || n2 < 2) return fail(-1, "sdfk_lcwg_eval: every axis needs at least 2 points");
    const long long n = (long long)n0 * n1 * n2, plane = (long long)n1 * n2;
    if (row_stride < n) return fail(-1, "sdfk_lcwg_eval: row stride smaller than the point count");
    const long long bx = (plane + 255) / 256, by = (n0 + SDFK_LCWG_SEG - 1) / SDFK_LCWG_SEG;
    if (bx > 0x7fffffffll || by > 65535) return fail(-1, "sdfk_lcwg_eval: grid too large");
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)bx, (unsigned)by);
    if (variant == 0)
        hipLaunchKernelGGL(sdfk_lcwg_kernel<0>, grid, dim3(256), 0, stream, d_uu, d_ww, g, w, d, sign_kind, sign_value, d_sign,
                           d_vec, (long long)row_stride);
    else if (variant == 1)
        hipLaunchKernelGGL(sdfk_lcwg_kernel<1>, grid, dim3(256), 0, stream, d_uu, d_ww, g, w, d, sign_kind, sign_value, d_sign,
                           d_vec, (long long)row_stride);
    else
        hipLaunchKernelGGL(sdfk_lcwg_kernel<2>, grid, dim3(256), 0, stream, d_uu, d_ww, g, w, d, sign_kind, sign_value, d_sign,
                           d_vec, (long long)row_stride);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_lcwg_eval: ") + hipGetErrorString(e));
    return 0;
}

// lcwg1_2d_old / lcwg1_p1_old / lcwg1_m1_old (:39-124): a straight guide along x, pointwise
__global__ __launch_bounds__(256) void sdfk_lcwg_old_kernel(int variant, const float* __restrict__ r, long long r_stride,
                                                             const float* __restrict__ uu, long long n, double w, double d,
                                                             float* __restrict__ out, long long stride) {
    const long long p = (long long)sdfk_bx() * 256 + sdfk_tx();
    if (p >= n) return;
    const double y = (double)r[r_stride + p], z = (double)r[2 * r_stride + p];
    const double qq = fmin(fmax((double)uu[p], 0.0), 1.0);
    double ox = 1.0, oy = 0.0, oz = 0.0;
    if (fabs(y) <= w / 2) {
        const double c = -cos(M_PI * qq), l2 = -sin(M_PI * qq);
        if (variant == 0) {
            ox = c;
            oy = l2;
        } else {
            double alpha = atan2(2.0 * z / (d * d), 8.0 * y / (w * w));
            if (variant == 2) alpha = -alpha;
            ox = c;
            oy = l2 * cos(alpha);
            oz = l2 * sin(alpha);
        }
        const double m = sqrt(ox * ox + oy * oy + oz * oz);    // the reference divides without a zero test
        ox = ox / m;
        oy = oy / m;
        oz = oz / m;
    }
    out[p] = (float)ox;
    out[stride + p] = (float)oy;
    out[2 * stride + p] = (float)oz;
}

extern "C" int sdfk_lcwg_old_eval(int variant, const float* d_r, int64_t r_stride, const float* d_uu, int64_t n, double w,
                                  double d, float* d_vec, int64_t row_stride, void* stream_) {
    if (variant < 0 || variant > 2) return fail(-1, "sdfk_lcwg_old_eval: variant must be 0 (2D), 1 (p1) or 2 (m1)");
    if (!d_r || !d_uu || !d_vec || n < 0) return fail(-1, "sdfk_lcwg_old_eval: bad arguments");
    if (r_stride < n || row_stride < n) return fail(-1, "sdfk_lcwg_old_eval: row stride smaller than the point count");
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(sdfk_lcwg_old_kernel, dim3(blocks256(n)), dim3(256), 0, stream, variant, d_r, (long long)r_stride, d_uu,
                       (long long)n, w, d, d_vec, (long long)row_stride);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_lcwg_old_eval: ") + hipGetErrorString(e));
    return 0;
}
