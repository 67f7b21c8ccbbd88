// level_ao.hip -- ambient occlusion of surface points from the dense level grid: 64 rays per point marched through the trilinear field.
//
// include/shapeclipper_hip.h states the rule operation by operation; tests/level_ao_ref.py restates it in numpy and the GPU tests
// compare bit for bit, so this file is built without contraction (Makefile) and keeps the stated order.
// One wave64 is one point, one lane one direction: __ballot is the mask and a __shfl_xor butterfly the two sums.  A first launch
// writes the bit volume of the cells that have a corner below iso; the march tests a sample's bit (one cached 4-byte load) before it
// loads the cell's 8 corners.  No atomics, no LDS, no wait on another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shapeclipper_hip.h"

namespace sc_ao {

constexpr int THREADS = 256;                  // 4 waves = 4 points a workgroup
constexpr int WAVES = THREADS / 64;
constexpr int MAX_IMAGES = 65535;
constexpr long long MAX_POINTS = 1LL << 30;

__host__ __device__ inline int words_z(int S) { return (S - 1 + 31) >> 5; }

// thread = one word: cells (x, y, 32 w .. 32 w + 31) of image b.  A cell's bit is set when one of its 8 corners is < iso.
__global__ void __launch_bounds__(THREADS) cell_bits_kernel(const float* __restrict__ level, int S, int WZ, long long words_per_image,
                                                            float iso, uint32_t* __restrict__ bits) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= words_per_image) return;
    const int b = blockIdx.y;
    const int C = S - 1;
    const int w = (int)(t % WZ);
    const long long row = t / WZ;
    const int y = (int)(row % C), x = (int)(row / C);
    const float* base = level + (long long)b * S * S * S;
    const float* c00 = base + ((long long)x * S + y) * S;
    const float* c01 = c00 + S;                               // (x, y + 1)
    const float* c10 = c00 + (long long)S * S;                // (x + 1, y)
    const float* c11 = c10 + S;
    const int z0 = 32 * w;
    const int z_end = min(z0 + 32, C);                        // cells z0 .. z_end - 1 read grid points z0 .. z_end <= S - 1
    auto below = [&](int z) { return c00[z] < iso || c01[z] < iso || c10[z] < iso || c11[z] < iso; };
    uint32_t word = 0u;
    bool lo = below(z0);
    for (int z = z0; z < z_end; ++z) {
        const bool hi = below(z + 1);
        if (lo || hi) word |= 1u << (z - z0);
        lo = hi;
    }
    bits[(long long)b * words_per_image + t] = word;
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

__device__ __forceinline__ float tree_sum(float a) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) a = a + __shfl_xor(a, m, 64);
    return a;                                                 // lane 0: the pairwise tree of the header
}

__device__ __forceinline__ bool finite3(float a, float b, float c) {
    return fabsf(a) < INFINITY && fabsf(b) < INFINITY && fabsf(c) < INFINITY;      // false for NaN
}

// wave = point, lane = direction
template <bool SKIP>
__global__ void __launch_bounds__(THREADS) march_kernel(const float* __restrict__ level, const float* __restrict__ points,
                                                        const float* __restrict__ normals, const int32_t* __restrict__ image,
                                                        const float* __restrict__ dirs, const uint32_t* __restrict__ bits, int n_images,
                                                        int S, long long n_points, float step, float bias, float iso, int n_steps,
                                                        float* __restrict__ ao, long long* __restrict__ mask, int32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (n >= n_points) return;                                // the whole wave
    const int b = image[n];
    const float px = points[3 * n], py = points[3 * n + 1], pz = points[3 * n + 2];
    const float nx = normals[3 * n], ny = normals[3 * n + 1], nz = normals[3 * n + 2];
    const bool bad_image = b < 0 || b >= n_images;
    bool open = true;
    float w = 0.0f;
    if (!bad_image && finite3(px, py, pz) && finite3(nx, ny, nz)) {
        const float Dx = dirs[3 * lane], Dy = dirs[3 * lane + 1], Dz = dirs[3 * lane + 2];
        const float dn = (Dx * nx + Dy * ny) + Dz * nz;
        const bool flip = dn < 0.0f;
        const float dx = flip ? -Dx : Dx, dy = flip ? -Dy : Dy, dz = flip ? -Dz : Dz;
        w = fabsf(dn);
        const float p0x = px + bias * nx, p0y = py + bias * ny, p0z = pz + bias * nz;
        const float top = (float)(S - 1);
        const int C = S - 1, WZ = words_z(S);
        const float* grid = level + (long long)b * S * S * S;
        const uint32_t* cells = SKIP ? bits + (long long)b * C * C * WZ : nullptr;
        for (int s = 1; s <= n_steps; ++s) {
            const float t = (float)s * step;
            const float qx = p0x + t * dx, qy = p0y + t * dy, qz = p0z + t * dz;
            if (!(qx >= 0.0f && qx <= top) || !(qy >= 0.0f && qy <= top) || !(qz >= 0.0f && qz <= top)) break;      // OPEN
            const int ix = min((int)floorf(qx), S - 2), iy = min((int)floorf(qy), S - 2), iz = min((int)floorf(qz), S - 2);
            if (SKIP) {
                const uint32_t word = cells[((long long)ix * C + iy) * WZ + (iz >> 5)];
                if (!((word >> (iz & 31)) & 1u)) continue;
            }
            const float* c = grid + ((long long)ix * S + iy) * S + iz;
            const long long sy = S, sx = (long long)S * S;
            const float v000 = c[0], v001 = c[1], v010 = c[sy], v011 = c[sy + 1];
            const float v100 = c[sx], v101 = c[sx + 1], v110 = c[sx + sy], v111 = c[sx + sy + 1];
            if (!SKIP) {
                const bool any = v000 < iso || v001 < iso || v010 < iso || v011 < iso || v100 < iso || v101 < iso || v110 < iso || v111 < iso;
                if (!any) continue;
            }
            const float fx = qx - (float)ix, fy = qy - (float)iy, fz = qz - (float)iz;
            const float u00 = lerp(v000, v001, fz), u01 = lerp(v010, v011, fz), u10 = lerp(v100, v101, fz), u11 = lerp(v110, v111, fz);
            const float u0 = lerp(u00, u01, fy), u1 = lerp(u10, u11, fy);
            if (lerp(u0, u1, fx) < iso) {
                open = false;                                 // CLOSED
                break;
            }
        }
    }
    const unsigned long long open_bits = __ballot(open);
    const float W = tree_sum(w);
    const float V = tree_sum(open ? w : 0.0f);
    if (lane == 0) {
        const bool ok = W > 0.0f;                             // false for the rows above (w = 0 in every lane) and for NaN
        ao[n] = ok ? V / W : 1.0f;
        mask[n] = ok ? (long long)open_bits : -1LL;
        if (bad_image) *bad = 1;
    }
}

}  // namespace sc_ao

extern "C" long long sc_level_ao_scratch_bytes(int n_images, int n_axis) {
    using namespace sc_ao;
    if (n_images < 1 || n_images > MAX_IMAGES || n_axis < 2 || n_axis > 1024) return -1;
    const long long C = n_axis - 1;
    return 4LL * n_images * C * C * words_z(n_axis);
}

extern "C" int sc_level_ambient_occlusion(const float* level, const float* points, const float* normals, const int32_t* image,
                                          const float* dirs, int n_images, int n_axis, long long n_points, float step, float bias, float iso,
                                          int n_steps, int cell_skip, void* scratch, float* ao, long long* mask, int32_t* bad,
                                          void* stream) {
    using namespace sc_ao;
    if (n_images < 1 || n_images > MAX_IMAGES || n_axis < 2 || n_axis > 1024 || n_steps < 1 || n_steps > SC_LEVEL_AO_MAX_STEPS ||
        n_points > MAX_POINTS)
        return (int)hipErrorInvalidValue;
    if (n_points <= 0) return 0;
    if (!level || !points || !normals || !image || !dirs || !ao || !mask || !bad) return (int)hipErrorInvalidValue;
    if (cell_skip && (!scratch || ((uintptr_t)scratch & 3))) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipError_t err = hipMemsetAsync(bad, 0, sizeof(int32_t), st);
    if (err != hipSuccess) return (int)err;
    const int S = n_axis;
    const dim3 block(THREADS);
    const dim3 grid((unsigned int)((n_points + WAVES - 1) / WAVES));
    if (cell_skip) {
        const int WZ = words_z(S);
        const long long words = (long long)(S - 1) * (S - 1) * WZ;
        const dim3 bgrid((unsigned int)((words + THREADS - 1) / THREADS), (unsigned int)n_images);
        hipLaunchKernelGGL(cell_bits_kernel, bgrid, block, 0, st, level, S, WZ, words, iso, (uint32_t*)scratch);
        hipLaunchKernelGGL(march_kernel<true>, grid, block, 0, st, level, points, normals, image, dirs, (const uint32_t*)scratch,
                           n_images, S, n_points, step, bias, iso, n_steps, ao, mask, bad);
    } else {
        hipLaunchKernelGGL(march_kernel<false>, grid, block, 0, st, level, points, normals, image, dirs, (const uint32_t*)nullptr,
                           n_images, S, n_points, step, bias, iso, n_steps, ao, mask, bad);
    }
    return (int)hipGetLastError();
}
