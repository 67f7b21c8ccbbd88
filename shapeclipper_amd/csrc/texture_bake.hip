// texture_bake.hip -- per-triangle texture atlas: the query points of the atlas texels, the uint8 atlases, and the bilinear look-up.
//
// include/shapeclipper_hip.h states the layout and every expression operation by operation; tests/texture_ref.py restates them in numpy
// and the GPU tests compare bit for bit, so this file is built without contraction (Makefile) and keeps the stated order.
// Every kernel is one thread per output element group with coalesced stores: the bake's cost is the two network chains between
// sc_texture_queries and sc_texture_pack (256 B of feature tile per texel against 12 B of query), not these.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shapeclipper_hip.h"

namespace sc_tex {

constexpr int THREADS = 256;
constexpr int MAX_IMAGES = 65535;             // gridDim.y

__host__ __device__ inline bool atlas_ok(int A) { return A >= 64 && A <= 8192 && (A & (A - 1)) == 0; }

// the position of texel (i, j) of half h of face `face` of the image whose faces start at fbase and whose vertices start at vbase
__device__ __forceinline__ void texel_query(const float* __restrict__ verts, const int32_t* __restrict__ faces, long long fbase,
                                            long long vbase, long long n_verts, long long face, int h, int i, int j, int T, float lo,
                                            float scale, float out[3]) {
    const float d = (float)(T - 3);
    const float b1 = (h ? (float)(T - 1 - i) : (float)i) / d;
    const float b2 = (h ? (float)(T - 1 - j) : (float)j) / d;
    const float b0 = (1.0f - b1) - b2;
    const int32_t* fv = faces + 3 * (fbase + face);
    const float* v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        long long vi = vbase + (long long)fv[k];
        vi = vi < 0 ? 0 : (vi >= n_verts ? n_verts - 1 : vi);         // never outside verts
        v[k] = verts + 3 * vi;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = (b0 * v[0][a] + b1 * v[1][a]) + b2 * v[2][a];
        out[a] = lo + p * scale;
    }
}

// grid (ceil(rows A / THREADS), n_images): thread = texel y A + x of image blockIdx.y
__global__ void __launch_bounds__(THREADS) queries_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                          const long long* __restrict__ v_start, const long long* __restrict__ f_start,
                                                          const long long* __restrict__ f_count, long long n_verts, int A, int log2A, int T,
                                                          int n, float lo, float scale, long long per_image, long long image_stride,
                                                          float* __restrict__ query, int32_t* __restrict__ face_of_texel) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= per_image) return;
    const int b = blockIdx.y;
    const int x = (int)(t & (A - 1)), y = (int)(t >> log2A);
    const long long F = f_count[b], fbase = f_start[b], vbase = v_start[b];
    const int cx = x / T, cy = y / T;                 // cy < n: rows <= n T
    const int i = x - cx * T, j = y - cy * T;
    const int h = (i + j <= T - 1) ? 0 : 1;
    const long long face = 2 * ((long long)cy * n + cx) + h;
    const bool used = cx < n && face < F;
    float p[3] = {lo, lo, lo};
    if (used)
        texel_query(verts, faces, fbase, vbase, n_verts, face, h, i, j, T, lo, scale, p);
    else if (F > 0)
        texel_query(verts, faces, fbase, vbase, n_verts, 0, 0, 0, 0, T, lo, scale, p);
    float* q = query + 3 * ((long long)b * image_stride + t);
    q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    face_of_texel[(long long)b * per_image + t] = used ? (int32_t)face : -1;
}

__device__ __forceinline__ uint32_t unit_byte(float v) {
    if (v != v) return 0u;                                            // NaN
    const float c = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    return (uint32_t)(c * 255.0f);                                    // truncation, c * 255 in [0, 255]
}

// grid (A A / (4 THREADS), n_images): thread = texels [4 g, 4 g + 4) of the image's full atlas (one row: A is a multiple of 4)
__global__ void __launch_bounds__(THREADS) pack_kernel(const float* __restrict__ rgb, const float* __restrict__ normal,
                                                       const int32_t* __restrict__ face_of_texel, int A, long long per_image,
                                                       uint8_t* __restrict__ atlas_rgb, uint8_t* __restrict__ atlas_normal) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
    const long long full = (long long)A * A;
    const long long t0 = 4 * g;
    if (t0 >= full) return;
    const int b = blockIdx.y;
    uint8_t c[12], m[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long t = t0 + k;
        const bool used = t < per_image && face_of_texel[(long long)b * per_image + t] >= 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            uint32_t cb = 127u, nb = 127u;
            if (used) {
                const long long src = 3 * ((long long)b * per_image + t) + a;
                cb = unit_byte(rgb[src]);
                nb = unit_byte((normal[src] + 1.0f) * 0.5f);
            }
            c[3 * k + a] = (uint8_t)cb;
            m[3 * k + a] = (uint8_t)nb;
        }
    }
    uint32_t* oc = reinterpret_cast<uint32_t*>(atlas_rgb + 3 * ((long long)b * full + t0));        // 12 g bytes past a 4-aligned base
    uint32_t* on = reinterpret_cast<uint32_t*>(atlas_normal + 3 * ((long long)b * full + t0));
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        oc[w] = (uint32_t)c[4 * w] | ((uint32_t)c[4 * w + 1] << 8) | ((uint32_t)c[4 * w + 2] << 16) | ((uint32_t)c[4 * w + 3] << 24);
        on[w] = (uint32_t)m[4 * w] | ((uint32_t)m[4 * w + 1] << 8) | ((uint32_t)m[4 * w + 2] << 16) | ((uint32_t)m[4 * w + 3] << 24);
    }
}

template <typename TEXEL>
__device__ __forceinline__ float texel(const TEXEL* __restrict__ atlas, long long at) { return (float)atlas[at]; }

// floor(x) as a column / row pair clamped to [0, A-1]; Inf and NaN land inside as well (fminf / fmaxf drop a NaN operand)
__device__ __forceinline__ void clamp_pair(float x0f, int A, int& lo_i, int& hi_i) {
    const int x0 = (int)fmaxf(fminf(x0f, (float)A), -1.0f);          // in [-1, A]
    lo_i = x0 < 0 ? 0 : (x0 > A - 1 ? A - 1 : x0);
    hi_i = x0 + 1 < 0 ? 0 : (x0 + 1 > A - 1 ? A - 1 : x0 + 1);
}

// thread = output element (point, channel)
template <typename TEXEL>
__global__ void __launch_bounds__(THREADS) sample_kernel(const TEXEL* __restrict__ atlas, const float* __restrict__ uv,
                                                         const int32_t* __restrict__ image_of_point, long long n_out, int n_images, int A,
                                                         int C, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= n_out) return;
    const long long pt = e / C;
    const int ch = (int)(e - pt * C);
    int b = image_of_point[pt];
    b = b < 0 ? 0 : (b >= n_images ? n_images - 1 : b);
    const float fA = (float)A;
    const float x = uv[2 * pt] * fA - 0.5f;
    const float y = (1.0f - uv[2 * pt + 1]) * fA - 0.5f;
    const float x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    int xa, xb, ya, yb;
    clamp_pair(x0f, A, xa, xb);
    clamp_pair(y0f, A, ya, yb);
    const long long base = (long long)b * A * A;
    const float t00 = texel(atlas, (base + (long long)ya * A + xa) * C + ch);
    const float t10 = texel(atlas, (base + (long long)ya * A + xb) * C + ch);
    const float t01 = texel(atlas, (base + (long long)yb * A + xa) * C + ch);
    const float t11 = texel(atlas, (base + (long long)yb * A + xb) * C + ch);
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float top = gx * t00 + fx * t10;
    const float bot = gx * t01 + fx * t11;
    out[e] = top * gy + bot * fy;
}

}  // namespace sc_tex

extern "C" int sc_texture_queries(const float* verts, const int32_t* faces, const long long* v_start, const long long* f_start,
                                  const long long* f_count, int n_images, long long n_verts, long long n_faces, int atlas, int texels,
                                  double lo, double hi, int n_axis, int rows, long long image_stride, float* query,
                                  int32_t* face_of_texel, void* stream) {
    using namespace sc_tex;
    if (n_images > MAX_IMAGES || texels < 4 || texels > 32 || !atlas_ok(atlas) || rows < 0 || rows > atlas || n_axis < 2 ||
        n_verts < 0 || n_faces < 0)
        return (int)hipErrorInvalidValue;
    const long long per_image = (long long)rows * atlas;
    if (image_stride < per_image) return (int)hipErrorInvalidValue;
    if (n_images <= 0 || rows == 0) return 0;
    if (!v_start || !f_start || !f_count || !query || !face_of_texel) return (int)hipErrorInvalidValue;
    if (n_faces > 0 && (!verts || !faces || n_verts == 0)) return (int)hipErrorInvalidValue;
    int log2A = 0;
    while ((1 << log2A) < atlas) ++log2A;
    const float scale = (float)((hi - lo) / (double)(n_axis - 1));
    const dim3 grid((unsigned int)((per_image + THREADS - 1) / THREADS), (unsigned int)n_images), block(THREADS);
    hipLaunchKernelGGL(queries_kernel, grid, block, 0, (hipStream_t)stream, verts, faces, v_start, f_start, f_count, n_verts, atlas,
                       log2A, texels, atlas / texels, (float)lo, scale, per_image, image_stride, query, face_of_texel);
    return (int)hipGetLastError();
}

extern "C" int sc_texture_pack(const float* rgb, const float* normal, const int32_t* face_of_texel, int n_images, int atlas, int rows,
                               unsigned char* atlas_rgb, unsigned char* atlas_normal, void* stream) {
    using namespace sc_tex;
    if (n_images > MAX_IMAGES || !atlas_ok(atlas) || rows < 0 || rows > atlas) return (int)hipErrorInvalidValue;
    if (n_images <= 0) return 0;
    if (!atlas_rgb || !atlas_normal || ((uintptr_t)atlas_rgb & 3) || ((uintptr_t)atlas_normal & 3)) return (int)hipErrorInvalidValue;
    if (rows > 0 && (!rgb || !normal || !face_of_texel)) return (int)hipErrorInvalidValue;
    const long long groups = (long long)atlas * atlas / 4;
    const dim3 grid((unsigned int)((groups + THREADS - 1) / THREADS), (unsigned int)n_images), block(THREADS);
    hipLaunchKernelGGL(pack_kernel, grid, block, 0, (hipStream_t)stream, rgb, normal, face_of_texel, atlas, (long long)rows * atlas,
                       (uint8_t*)atlas_rgb, (uint8_t*)atlas_normal);
    return (int)hipGetLastError();
}

extern "C" int sc_texture_sample(const void* atlas_data, int is_u8, const float* uv, const int32_t* image_of_point, long long n_points,
                                 int n_images, int atlas, int channels, float* out, void* stream) {
    using namespace sc_tex;
    if (n_images > MAX_IMAGES || !atlas_ok(atlas) || channels < 1 || channels > 16 || n_points > (1LL << 40))
        return (int)hipErrorInvalidValue;
    if (n_points <= 0) return 0;
    if (n_images <= 0 || !atlas_data || !uv || !image_of_point || !out) return (int)hipErrorInvalidValue;
    const long long n_out = n_points * channels;
    const long long blocks = (n_out + THREADS - 1) / THREADS;
    if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned int)blocks), block(THREADS);
    if (is_u8)
        hipLaunchKernelGGL(sample_kernel<uint8_t>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)atlas_data, uv, image_of_point,
                           n_out, n_images, atlas, channels, out);
    else
        hipLaunchKernelGGL(sample_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)atlas_data, uv, image_of_point,
                           n_out, n_images, atlas, channels, out);
    return (int)hipGetLastError();
}
