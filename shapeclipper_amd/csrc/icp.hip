// icp.hip -- the fit, the apply and the objective of the evaluation's similarity ICP (ops.icp_fit / icp_apply / icp_align).  The search
// between them is the Chamfer forward (chamfer.hip / chamfer_grid.hip), untouched.  include/shapeclipper_hip.h states the definition,
// the order of every sum included; tests/icp_ref.py restates it in numpy.  Built without contraction: every operation rounds once.
//
// All accumulation is float64.  A sum over the pairs of one half (source -> target, target -> source) goes in three fixed stages:
//   thread   t of a workgroup adds its chunk's pairs t, t + 256, t + 512, t + 768 in that order (a pair past the half's end adds +0.0);
//   workgroup: each wave folds its 64 lanes with v += shfl_down(v, 32), 16, 8, 4, 2, 1; the four wave sums are added in wave order;
//   image    : the chunk partials of a half are added in ascending chunk number by one lane.
// Nothing is accumulated by an atomic; a partial is written once by a plain vector store and read by a later launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shapeclipper_hip.h"

namespace sc_icp {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int PER_THREAD = 4;
constexpr int CHUNK = THREADS * PER_THREAD;       // SC_ICP_CHUNK pairs per workgroup
constexpr int MEAN_K = 6;                         // sum p (3), sum q (3)
constexpr int COV_K = 10;                         // sum (q - qm)(p - pm)^T row-major (9), sum |p - pm|^2
constexpr int WS_K = MEAN_K + COV_K;              // doubles per chunk in the workspace
constexpr int MAX_IMAGES = 65535;
constexpr int JACOBI_SWEEPS = 30;

static_assert(CHUNK == SC_ICP_CHUNK, "the header states the chunk size");

__host__ __device__ __forceinline__ int chunks_of(int n) { return (n + CHUNK - 1) / CHUNK; }

// Pair k of a half: half 0 is (src[k], dst[idx1[k]]), half 1 is (src[idx2[k]], dst[k]).  An index outside its cloud gives a NaN pair,
// which makes the image's sums non-finite (the fit then keeps the previous transform) instead of a read out of bounds.
__device__ __forceinline__ void load_pair(const float* __restrict__ src, const float* __restrict__ dst, const int* __restrict__ idx1,
                                          const int* __restrict__ idx2, int n, int m, int half, int k, double p[3], double q[3]) {
    int i, j;
    if (half == 0) { i = k; j = idx1[k]; } else { j = k; i = idx2[k]; }
    if ((unsigned int)i < (unsigned int)n && (unsigned int)j < (unsigned int)m) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { p[c] = (double)src[(long long)i * 3 + c]; q[c] = (double)dst[(long long)j * 3 + c]; }
    } else {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
        for (int c = 0; c < 3; ++c) { p[c] = nan; q[c] = nan; }
    }
}

// The workgroup stage: v[k] of 256 threads -> out[k], written by thread k.  lds holds WAVES * K doubles.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* lds, double* __restrict__ out) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) lds[wave * K + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        out[k] = ((lds[0 * K + k] + lds[1 * K + k]) + lds[2 * K + k]) + lds[3 * K + k];
    }
}

// The image stage for component k of an image's workspace rows: (S1 / n + S2 / m) / 2, S1 over the chunks of half 0 and S2 over those of
// half 1, each in ascending chunk number.  (Per-half division: N equal fp32 values sum exactly and divide back to the value itself.)
__device__ __forceinline__ double image_mean(const double* __restrict__ rows, int stride, int k, int c1, int c2, int n, int m) {
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < c1; ++c) s1 += rows[(long long)c * stride + k];
    for (int c = c1; c < c1 + c2; ++c) s2 += rows[(long long)c * stride + k];
    return (s1 / (double)n + s2 / (double)m) * 0.5;
}

// grid (c1 + c2, n_images): sums of p and q over one chunk -> ws[image][chunk][0..5]
__global__ void __launch_bounds__(THREADS) mean_partial_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                               const int* __restrict__ idx1, const int* __restrict__ idx2, int n, int m,
                                                               double* __restrict__ ws) {
    __shared__ double lds[WAVES * MEAN_K];
    const int c1 = chunks_of(n), c2 = chunks_of(m), b = blockIdx.y;
    const int chunk = blockIdx.x, half = chunk < c1 ? 0 : 1;
    const int first = (half == 0 ? chunk : chunk - c1) * CHUNK, count = half == 0 ? n : m;
    src += (long long)b * n * 3; dst += (long long)b * m * 3; idx1 += (long long)b * n; idx2 += (long long)b * m;
    double v[MEAN_K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < PER_THREAD; ++r) {
        const int k = first + r * THREADS + (int)threadIdx.x;
        if (k < count) {
            double p[3], q[3];
            load_pair(src, dst, idx1, idx2, n, m, half, k, p, q);
#pragma unroll
            for (int c = 0; c < 3; ++c) { v[c] += p[c]; v[3 + c] += q[c]; }
        }
    }
    block_sum<MEAN_K>(v, lds, ws + ((long long)b * (c1 + c2) + chunk) * WS_K);
}

// grid (c1 + c2, n_images): the centred sums over one chunk -> ws[image][chunk][6..15]
__global__ void __launch_bounds__(THREADS) cov_partial_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                              const int* __restrict__ idx1, const int* __restrict__ idx2, int n, int m,
                                                              double* __restrict__ ws) {
    __shared__ double lds[WAVES * COV_K];
    __shared__ double mean[MEAN_K];
    const int c1 = chunks_of(n), c2 = chunks_of(m), b = blockIdx.y;
    const int chunk = blockIdx.x, half = chunk < c1 ? 0 : 1;
    const int first = (half == 0 ? chunk : chunk - c1) * CHUNK, count = half == 0 ? n : m;
    double* rows = ws + (long long)b * (c1 + c2) * WS_K;
    if (threadIdx.x < MEAN_K) mean[threadIdx.x] = image_mean(rows, WS_K, threadIdx.x, c1, c2, n, m);
    __syncthreads();
    const double pm[3] = {mean[0], mean[1], mean[2]}, qm[3] = {mean[3], mean[4], mean[5]};
    src += (long long)b * n * 3; dst += (long long)b * m * 3; idx1 += (long long)b * n; idx2 += (long long)b * m;
    double v[COV_K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < PER_THREAD; ++r) {
        const int k = first + r * THREADS + (int)threadIdx.x;
        if (k < count) {
            double p[3], q[3];
            load_pair(src, dst, idx1, idx2, n, m, half, k, p, q);
            const double dp[3] = {p[0] - pm[0], p[1] - pm[1], p[2] - pm[2]};
            const double dq[3] = {q[0] - qm[0], q[1] - qm[1], q[2] - qm[2]};
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) v[i * 3 + j] += dq[i] * dp[j];
            v[9] += (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2];
        }
    }
    block_sum<COV_K>(v, lds, rows + (long long)chunk * WS_K + MEAN_K);
}

struct Vec { double x, y, z; };
__device__ __forceinline__ double dot(const Vec& a, const Vec& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ Vec cross(const Vec& a, const Vec& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ Vec scaled(const Vec& a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ void swap(Vec& a, Vec& b) { const Vec t = a; a = b; b = t; }

// One step of the one-sided Jacobi method: a right rotation that makes columns ap, aq of H V orthogonal (the same rotation on V's).
__device__ __forceinline__ bool rotate(Vec& ap, Vec& aq, Vec& vp, Vec& vq) {
    const double alpha = dot(ap, ap), beta = dot(aq, aq), gamma = dot(ap, aq);
    if (gamma == 0.0 || fabs(gamma) <= 1.0e-16 * (sqrt(alpha) * sqrt(beta))) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    const Vec np = {c * ap.x - s * aq.x, c * ap.y - s * aq.y, c * ap.z - s * aq.z};
    const Vec nq = {s * ap.x + c * aq.x, s * ap.y + c * aq.y, s * ap.z + c * aq.z};
    const Vec mp = {c * vp.x - s * vq.x, c * vp.y - s * vq.y, c * vp.z - s * vq.z};
    const Vec mq = {s * vp.x + c * vq.x, s * vp.y + c * vq.y, s * vp.z + c * vq.z};
    ap = np; aq = nq; vp = mp; vq = mq;
    return true;
}

__device__ __forceinline__ bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for NaN and Inf

// grid n_images, one wave each: lanes 0..15 add the chunk partials of their component, lane 0 solves and writes.
__global__ void __launch_bounds__(64) solve_kernel(const double* __restrict__ ws, int n, int m, int with_scale,
                                                   const double* prev_transform, const double* prev_scale,
                                                   double* transform, double* scale) {
    __shared__ double sum[WS_K];
    const int c1 = chunks_of(n), c2 = chunks_of(m), b = blockIdx.x;
    if (threadIdx.x < WS_K) sum[threadIdx.x] = image_mean(ws + (long long)b * (c1 + c2) * WS_K, WS_K, threadIdx.x, c1, c2, n, m);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* T = transform + (long long)b * 16;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < WS_K; ++k) ok = ok && finite(sum[k]);
    const Vec pm = {sum[0], sum[1], sum[2]}, qm = {sum[3], sum[4], sum[5]};
    const double var_p = sum[15];
    ok = ok && var_p > 0.0;
    // H = U D V^T by one-sided Jacobi: rotations from the right until the columns of A = H V are orthogonal; then D = their norms
    Vec a0 = {sum[6], sum[9], sum[12]}, a1 = {sum[7], sum[10], sum[13]}, a2 = {sum[8], sum[11], sum[14]};     // columns of H
    Vec v0 = {1.0, 0.0, 0.0}, v1 = {0.0, 1.0, 0.0}, v2 = {0.0, 0.0, 1.0};
    if (ok) {
        for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
            bool any = rotate(a0, a1, v0, v1);
            any = rotate(a0, a2, v0, v2) || any;
            any = rotate(a1, a2, v1, v2) || any;
            if (!any) break;
        }
    }
    double d0 = sqrt(dot(a0, a0)), d1 = sqrt(dot(a1, a1)), d2 = sqrt(dot(a2, a2));
    if (d0 < d1) { swap(a0, a1); swap(v0, v1); const double t = d0; d0 = d1; d1 = t; }
    if (d0 < d2) { swap(a0, a2); swap(v0, v2); const double t = d0; d0 = d2; d2 = t; }
    if (d1 < d2) { swap(a1, a2); swap(v1, v2); const double t = d1; d1 = d2; d2 = t; }
    ok = ok && finite(d0) && d1 > 1.0e-12 * d0;           // the rotation is undetermined at rank <= 1 (covers H = 0)
    double M[12], s = 1.0;
    if (ok) {
        const Vec u0 = scaled(a0, 1.0 / d0), u1 = scaled(a1, 1.0 / d1);
        const Vec un = cross(u0, u1), vn = cross(v0, v1);
        // U diag(1, 1, det U det V) V^T = u0 v0^T + u1 v1^T + (u0 x u1)(v0 x v1)^T: the third columns are +-(u0 x u1) and +-(v0 x v1), and
        // the two signs are the two determinants.  Their product is also the sign D's third entry takes in the scale.
        const double sign = dot(a2, un) * dot(v2, vn) < 0.0 ? -1.0 : 1.0;
        if (with_scale) s = ((d0 + d1) + sign * d2) / var_p;
        const double R[9] = {(u0.x * v0.x + u1.x * v1.x) + un.x * vn.x, (u0.x * v0.y + u1.x * v1.y) + un.x * vn.y, (u0.x * v0.z + u1.x * v1.z) + un.x * vn.z,
                             (u0.y * v0.x + u1.y * v1.x) + un.y * vn.x, (u0.y * v0.y + u1.y * v1.y) + un.y * vn.y, (u0.y * v0.z + u1.y * v1.z) + un.y * vn.z,
                             (u0.z * v0.x + u1.z * v1.x) + un.z * vn.x, (u0.z * v0.y + u1.z * v1.y) + un.z * vn.y, (u0.z * v0.z + u1.z * v1.z) + un.z * vn.z};
        const double qmv[3] = {qm.x, qm.y, qm.z};
        ok = finite(s);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            M[r * 4 + 0] = s * R[r * 3 + 0]; M[r * 4 + 1] = s * R[r * 3 + 1]; M[r * 4 + 2] = s * R[r * 3 + 2];
            M[r * 4 + 3] = qmv[r] - ((M[r * 4 + 0] * pm.x + M[r * 4 + 1] * pm.y) + M[r * 4 + 2] * pm.z);
#pragma unroll
            for (int c = 0; c < 4; ++c) ok = ok && finite(M[r * 4 + c]);
        }
    }
    if (ok) {
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = M[k];
        T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
        scale[b] = s;
    } else if (prev_transform != nullptr) {               // keep the previous transform (a plain copy; in place it rewrites the same bits)
        const double* P = prev_transform + (long long)b * 16;
        double keep[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) keep[k] = P[k];
        const double ks = prev_scale[b];
#pragma unroll
        for (int k = 0; k < 16; ++k) T[k] = keep[k];
        scale[b] = ks;
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
        scale[b] = 1.0;
    }
}

// grid (ceil(n / 256), n_images): out = fp32(((m0 x + m1 y) + m2 z) + t) per coordinate, in float64, one rounding to fp32 at the end
__global__ void __launch_bounds__(THREADS) apply_kernel(const float* __restrict__ src, const double* __restrict__ transform, int n,
                                                        float* __restrict__ out) {
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const double* T = transform + (long long)b * 16;
    const float* p = src + ((long long)b * n + i) * 3;
    float* o = out + ((long long)b * n + i) * 3;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (float)(((T[r * 4 + 0] * x + T[r * 4 + 1] * y) + T[r * 4 + 2] * z) + T[r * 4 + 3]);
}

// grid (c1 + c2, n_images): the sum of one chunk of dist1 (half 0) or dist2 (half 1) -> ws[image][chunk]
__global__ void __launch_bounds__(THREADS) objective_partial_kernel(const float* __restrict__ dist1, const float* __restrict__ dist2, int n,
                                                                    int m, double* __restrict__ ws) {
    __shared__ double lds[WAVES];
    const int c1 = chunks_of(n), c2 = chunks_of(m), b = blockIdx.y;
    const int chunk = blockIdx.x, half = chunk < c1 ? 0 : 1;
    const int first = (half == 0 ? chunk : chunk - c1) * CHUNK, count = half == 0 ? n : m;
    const float* d = half == 0 ? dist1 + (long long)b * n : dist2 + (long long)b * m;
    double v[1] = {0.0};
#pragma unroll
    for (int r = 0; r < PER_THREAD; ++r) {
        const int k = first + r * THREADS + (int)threadIdx.x;
        if (k < count) v[0] += (double)d[k];
    }
    block_sum<1>(v, lds, ws + (long long)b * (c1 + c2) + chunk);
}

// grid n_images, one lane each: objective[b * stride] = S1 / n + S2 / m, chunk partials in ascending chunk number
__global__ void __launch_bounds__(64) objective_finish_kernel(const double* __restrict__ ws, int n, int m, double* __restrict__ objective,
                                                              long long stride) {
    if (threadIdx.x != 0) return;
    const int c1 = chunks_of(n), c2 = chunks_of(m), b = blockIdx.x;
    objective[(long long)b * stride] = 2.0 * image_mean(ws + (long long)b * (c1 + c2), 1, 0, c1, c2, n, m);
}

__host__ inline bool sizes_ok(int n_images, int n, int m) { return n_images <= MAX_IMAGES && n >= 1 && m >= 1; }

}  // namespace sc_icp

extern "C" long long sc_icp_workspace_bytes(int n_images, int n, int m) {
    using namespace sc_icp;
    if (n_images <= 0) return 0;
    if (!sizes_ok(n_images, n, m)) return -1;
    return (long long)n_images * (chunks_of(n) + chunks_of(m)) * WS_K * (long long)sizeof(double);
}

extern "C" int sc_icp_fit(const float* src, const float* dst, const int* idx1, const int* idx2, int n_images, int n, int m, int with_scale,
                          const double* prev_transform, const double* prev_scale, double* workspace, double* transform, double* scale,
                          void* stream) {
    using namespace sc_icp;
    if (n_images <= 0) return 0;
    if (!sizes_ok(n_images, n, m) || !src || !dst || !idx1 || !idx2 || !workspace || !transform || !scale) return (int)hipErrorInvalidValue;
    if ((prev_transform == nullptr) != (prev_scale == nullptr)) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned int)(chunks_of(n) + chunks_of(m)), (unsigned int)n_images), block(THREADS);
    hipLaunchKernelGGL(mean_partial_kernel, grid, block, 0, s, src, dst, idx1, idx2, n, m, workspace);
    hipLaunchKernelGGL(cov_partial_kernel, grid, block, 0, s, src, dst, idx1, idx2, n, m, workspace);
    hipLaunchKernelGGL(solve_kernel, dim3((unsigned int)n_images), dim3(64), 0, s, (const double*)workspace, n, m, with_scale ? 1 : 0,
                       prev_transform, prev_scale, transform, scale);
    return (int)hipGetLastError();
}

extern "C" int sc_icp_apply(const float* src, const double* transform, int n_images, int n, float* out, void* stream) {
    using namespace sc_icp;
    if (n_images <= 0) return 0;
    if (!sizes_ok(n_images, n, 1) || !src || !transform || !out) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned int)((n + THREADS - 1) / THREADS), (unsigned int)n_images), block(THREADS);
    hipLaunchKernelGGL(apply_kernel, grid, block, 0, (hipStream_t)stream, src, transform, n, out);
    return (int)hipGetLastError();
}

extern "C" int sc_icp_objective(const float* dist1, const float* dist2, int n_images, int n, int m, double* workspace, double* objective,
                                long long objective_stride, void* stream) {
    using namespace sc_icp;
    if (n_images <= 0) return 0;
    if (!sizes_ok(n_images, n, m) || !dist1 || !dist2 || !workspace || !objective || objective_stride < 1) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned int)(chunks_of(n) + chunks_of(m)), (unsigned int)n_images), block(THREADS);
    hipLaunchKernelGGL(objective_partial_kernel, grid, block, 0, s, dist1, dist2, n, m, workspace);
    hipLaunchKernelGGL(objective_finish_kernel, dim3((unsigned int)n_images), dim3(64), 0, s, (const double*)workspace, n, m, objective,
                       objective_stride);
    return (int)hipGetLastError();
}
