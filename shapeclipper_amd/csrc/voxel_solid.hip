// voxel_solid.hip -- the voxel solid of a point cloud and the volumetric IoU of two of them (ops.voxel_frame / voxel_solid / voxel_iou, the
// evaluation's iou.txt under --eval.iou).  include/shapeclipper_hip.h states every step operation by operation; tests/voxel_iou_ref.py
// restates it in numpy.  Built without contraction: every fp32 operation rounds once.
//
// solid_kernel: one workgroup per image, the whole job in LDS: workgroup barriers only, no other workgroup is waited for, no global
// memory is spun on, nothing is read back by the host, no float atomics.  A volume is one 64-bit word per (x, y) row, bit z.  LDS,
// dynamic, three volumes of R^2 words -- 96 KiB at R = 64 (above the 64 KiB default, so the launch raises the kernel's limit the way
// emd3d.hip does; a CU has 160 KiB):
//   A : the shell (64-bit integer LDS OR per point, after a plain read that skips the voxels already set), then D = the shell
//       dilated c times, then F = not E and the solid, eroded in place;
//   B, C : the separable passes' intermediate, then the exterior E of the Jacobi sweeps, read from one and written to the other.
// A sweep ORs a row with its four neighbour rows, masks it by `free` = not D and smears it along z inside the word to the fixed point
// (a Kogge-Stone fill: six doubling steps each way), so a z column costs one sweep, not R.  The loop ends when a sweep changes nothing:
// E only grows in a finite grid.  The changed flag is one of three LDS words in rotation: sweep k raises word k % 3, which every
// thread reads behind the sweep's barrier, and clears word (k + 1) % 3, which was last read behind the barrier of sweep k - 2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shapeclipper_hip.h"

namespace sc_vox {

typedef unsigned long long u64;

constexpr int MAX_RES = SC_VOXEL_MAX_RES;
constexpr int MAX_IMAGES = 65535;
constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;
constexpr int IOU_THREADS = 256;
constexpr int MAX_WORDS = 1 << 24;
constexpr int LDS_MAX = 3 * 8 * MAX_RES * MAX_RES;      // 98,304 bytes

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= 3.402823466e+38f; }      // false for NaN and Inf

// adds the lanes' v into *total (LDS): shuffles inside the wave, one integer LDS add per wave -- a sum of integers, any order
__device__ __forceinline__ void block_add(int* total, int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(total, v);
}

// the fixed point of  v |= ((v << 1) | (v >> 1)) & free  for v inside free: every run of free bits that holds a bit of v, whole
__device__ __forceinline__ u64 smear(u64 v, u64 free) {
    u64 up = v, down = v, pu = free, pd = free;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        up |= pu & (up << s);
        pu &= pu << s;
        down |= pd & (down >> s);
        pd &= pd >> s;
    }
    return up | down;
}

__global__ void __launch_bounds__(THREADS) frame_kernel(const float* __restrict__ a, const float* __restrict__ b, int n_a, int n_b, int R,
                                                     int m, float* __restrict__ origin, float* __restrict__ pitch) {
    __shared__ float s_lo[WAVES][3], s_hi[WAVES][3];
    __shared__ int s_bad;
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int cloud = 0; cloud < 2; ++cloud) {
        const int n = cloud ? n_b : n_a;
        const float* p = (cloud ? b : a) + (long long)img * n * 3;
        for (int k = tid; k < n; k += THREADS) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float v = p[3 * (long long)k + d];
                bad = bad || !finite(v);
                lo[d] = fminf(lo[d], v);
                hi[d] = fmaxf(hi[d], v);
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo[d] = fminf(lo[d], __shfl_xor(lo[d], off, 64));
            hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], off, 64));
        }
        if (lane == 0) { s_lo[wave][d] = lo[d]; s_hi[wave][d] = hi[d]; }
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (tid != 0) return;
    if (s_bad) {
        const float qnan = __uint_as_float(0x7fc00000u);
        origin[3 * img + 0] = qnan; origin[3 * img + 1] = qnan; origin[3 * img + 2] = qnan; pitch[img] = qnan;
        return;
    }
    for (int d = 0; d < 3; ++d)
        for (int w = 0; w < WAVES; ++w) { lo[d] = fminf(lo[d], s_lo[w][d]); hi[d] = fmaxf(hi[d], s_hi[w][d]); }
    const float side = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    const float pt = side == 0.f ? 1.0f : side / (float)(R - 2 * m);
    const float half = (float)R * 0.5f;
    for (int d = 0; d < 3; ++d) {
        const float centre = (lo[d] + hi[d]) * 0.5f;
        origin[3 * img + d] = centre - half * pt;
    }
    pitch[img] = pt;
}

__global__ void __launch_bounds__(THREADS) solid_kernel(const float* __restrict__ points, const float* __restrict__ origin,
                                                     const float* __restrict__ pitch, int n, int R, int c, long long* __restrict__ bits,
                                                     int* __restrict__ shell_out, int* __restrict__ solid_out, int* __restrict__ sweeps_out) {
    extern __shared__ u64 lds_raw[];
    const int W = R * R;
    u64* A = lds_raw;
    u64* Bf = A + W;
    u64* C = Bf + W;
    __shared__ int s_count[2], s_flag[3];

    const int img = blockIdx.x, tid = threadIdx.x;
    const int m = c + 1;
    const u64 mask = R == 64 ? ~0ull : (1ull << R) - 1ull;
    const float* p = points + (long long)img * n * 3;

    for (int i = tid; i < W; i += THREADS) A[i] = 0ull;
    if (tid == 0) { s_count[0] = 0; s_count[1] = 0; s_flag[0] = 0; s_flag[1] = 0; s_flag[2] = 0; }
    __syncthreads();

    // ---- shell: indices are clamped to [m, R - 1 - m], inside [0, R - 1] for every res and close the entry point lets through
    const float ox = origin[3 * img + 0], oy = origin[3 * img + 1], oz = origin[3 * img + 2], pt = pitch[img];
    if (finite(ox) && finite(oy) && finite(oz) && finite(pt) && pt > 0.f) {
        const float flo = (float)m, fhi = (float)(R - 1 - m);
        for (int k = tid; k < n; k += THREADS) {
            const float x = p[3 * (long long)k + 0], y = p[3 * (long long)k + 1], z = p[3 * (long long)k + 2];
            if (!finite(x) || !finite(y) || !finite(z)) continue;
            const int ix = (int)fminf(fmaxf(floorf((x - ox) / pt), flo), fhi);
            const int iy = (int)fminf(fmaxf(floorf((y - oy) / pt), flo), fhi);
            const int iz = (int)fminf(fmaxf(floorf((z - oz) / pt), flo), fhi);
            const u64 bit = 1ull << iz;
            u64* word = &A[ix * R + iy];
            if ((*(volatile u64*)word & bit) == 0ull) atomicOr(word, bit);
        }
    }
    __syncthreads();
    {
        int count = 0;
        for (int i = tid; i < W; i += THREADS) count += __popcll(A[i]);
        block_add(&s_count[0], count);
    }

    // ---- D = the shell dilated c times by the cube: z inside the word, y by the neighbouring words, x by the neighbouring rows
    for (int t = 0; t < c; ++t) {
        for (int i = tid; i < W; i += THREADS) { const u64 w = A[i]; A[i] = (w | (w << 1) | (w >> 1)) & mask; }
        __syncthreads();
        for (int i = tid; i < W; i += THREADS) {
            const int y = i % R;
            Bf[i] = A[i] | (y > 0 ? A[i - 1] : 0ull) | (y < R - 1 ? A[i + 1] : 0ull);
        }
        __syncthreads();
        for (int i = tid; i < W; i += THREADS) {
            const int x = i / R;
            A[i] = Bf[i] | (x > 0 ? Bf[i - R] : 0ull) | (x < R - 1 ? Bf[i + R] : 0ull);
        }
        __syncthreads();
    }

    // ---- exterior E: Jacobi sweeps from the border, cur -> nxt
    const u64 ends = 1ull | (1ull << (R - 1));
    for (int i = tid; i < W; i += THREADS) {
        const int x = i / R, y = i % R;
        const u64 free = ~A[i] & mask;
        Bf[i] = (x == 0 || x == R - 1 || y == 0 || y == R - 1) ? free : (free & ends);
    }
    __syncthreads();
    u64* cur = Bf;
    u64* nxt = C;
    int sweeps = 0;                                     // the same in every thread
    for (;;) {
        const int slot = sweeps % 3;
        if (tid == 0) s_flag[(sweeps + 1) % 3] = 0;
        bool changed = false;
        for (int i = tid; i < W; i += THREADS) {
            const int x = i / R, y = i % R;
            const u64 free = ~A[i] & mask, old = cur[i];
            u64 v = old;
            if (x > 0) v |= cur[i - R];
            if (x < R - 1) v |= cur[i + R];
            if (y > 0) v |= cur[i - 1];
            if (y < R - 1) v |= cur[i + 1];
            v = smear(v & free, free);
            nxt[i] = v;
            changed = changed || v != old;
        }
        if (changed) s_flag[slot] = 1;
        __syncthreads();
        ++sweeps;
        u64* const swap = cur; cur = nxt; nxt = swap;
        if (s_flag[slot] == 0) break;
    }

    // ---- F = not E; the solid = F eroded c times, the outside of the grid empty (every thread is behind the last sweep's barrier)
    for (int i = tid; i < W; i += THREADS) A[i] = ~cur[i] & mask;
    __syncthreads();
    for (int t = 0; t < c; ++t) {
        for (int i = tid; i < W; i += THREADS) { const u64 w = A[i]; A[i] = w & (w << 1) & (w >> 1); }
        __syncthreads();
        for (int i = tid; i < W; i += THREADS) {
            const int y = i % R;
            Bf[i] = A[i] & (y > 0 ? A[i - 1] : 0ull) & (y < R - 1 ? A[i + 1] : 0ull);
        }
        __syncthreads();
        for (int i = tid; i < W; i += THREADS) {
            const int x = i / R;
            A[i] = Bf[i] & (x > 0 ? Bf[i - R] : 0ull) & (x < R - 1 ? Bf[i + R] : 0ull);
        }
        __syncthreads();
    }
    {
        int count = 0;
        long long* out = bits + (long long)img * W;
        for (int i = tid; i < W; i += THREADS) { const u64 w = A[i]; out[i] = (long long)w; count += __popcll(w); }
        block_add(&s_count[1], count);
    }
    __syncthreads();
    if (tid == 0) { shell_out[img] = s_count[0]; solid_out[img] = s_count[1]; sweeps_out[img] = sweeps; }
}

__global__ void __launch_bounds__(IOU_THREADS) iou_kernel(const long long* __restrict__ bits_a, const long long* __restrict__ bits_b, int words,
                                                       int* __restrict__ inter, int* __restrict__ uni) {
    __shared__ int s_count[2];
    const int img = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { s_count[0] = 0; s_count[1] = 0; }
    __syncthreads();
    const long long* a = bits_a + (long long)img * words;
    const long long* b = bits_b + (long long)img * words;
    int n_and = 0, n_or = 0;
    for (int i = tid; i < words; i += IOU_THREADS) {
        const u64 x = (u64)a[i], y = (u64)b[i];
        n_and += __popcll(x & y);
        n_or += __popcll(x | y);
    }
    block_add(&s_count[0], n_and);
    block_add(&s_count[1], n_or);
    __syncthreads();
    if (tid == 0) { inter[img] = s_count[0]; uni[img] = s_count[1]; }
}

static bool bad_grid(int n_images, int res, int close) {
    return n_images > MAX_IMAGES || res < SC_VOXEL_MIN_RES || res > MAX_RES || close < 0 || close > SC_VOXEL_MAX_CLOSE;
}

}  // namespace sc_vox

extern "C" int sc_voxel_frame(const float* a, const float* b, int n_images, int n_a, int n_b, int res, int close, float* origin, float* pitch,
                              void* stream) {
    using namespace sc_vox;
    if (n_images <= 0) return 0;
    if (bad_grid(n_images, res, close) || n_a < 1 || n_b < 1 || !a || !b || !origin || !pitch) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(frame_kernel, dim3((unsigned int)n_images), dim3(THREADS), 0, (hipStream_t)stream, a, b, n_a, n_b, res, close + 1, origin,
                       pitch);
    return (int)hipGetLastError();
}

extern "C" int sc_voxel_solid(const float* points, const float* origin, const float* pitch, int n_images, int n, int res, int close, int64_t* bits,
                              int32_t* shell_voxels, int32_t* solid_voxels, int32_t* sweeps, void* stream) {
    using namespace sc_vox;
    if (n_images <= 0) return 0;
    if (bad_grid(n_images, res, close) || n < 1 || !points || !origin || !pitch || !bits || !shell_voxels || !solid_voxels || !sweeps)
        return (int)hipErrorInvalidValue;
    const int lds_bytes = 3 * 8 * res * res;
    (void)hipFuncSetAttribute((const void*)solid_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);   // per launch: the attribute is per device, no process-wide state
    hipLaunchKernelGGL(solid_kernel, dim3((unsigned int)n_images), dim3(THREADS), lds_bytes, (hipStream_t)stream, points, origin, pitch, n, res,
                       close, (long long*)bits, shell_voxels, solid_voxels, sweeps);
    return (int)hipGetLastError();
}

extern "C" int sc_voxel_iou(const int64_t* bits_a, const int64_t* bits_b, int n_images, int words, int32_t* inter, int32_t* uni, void* stream) {
    using namespace sc_vox;
    if (n_images <= 0) return 0;
    if (n_images > MAX_IMAGES || words < 1 || words > MAX_WORDS || !bits_a || !bits_b || !inter || !uni) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(iou_kernel, dim3((unsigned int)n_images), dim3(IOU_THREADS), 0, (hipStream_t)stream, (const long long*)bits_a,
                       (const long long*)bits_b, words, inter, uni);
    return (int)hipGetLastError();
}
