// clip_preprocess.hip -- the CLIP tower's input from a batch of Pix3D loader images, exactly as the reference builds it.
//
// Reference (CLIP-annotation mode): data/pix3d.py:278-289 composites the loader's RGBA image on the background colour, then
// torchvision's to_pil_image and openai/CLIP's _transform(n_px) (Resize(n_px, BICUBIC), CenterCrop(n_px), ToTensor, Normalize).
// Per image, with the host-built tables of data/clip_preprocess.py:
//   1. quantise: q = a >= 128 ? c : bg  (to_tensor, mask = a/255 > 0.5, composite, mul(255).byte(); bg < 0: no composite, q = c);
//   2. horizontal pass, source row r, cropped output column x:
//        t(r, x) = clip8((2^21 + sum_i q(r, hb[x].start + i) * hk[x][i]) >> 22)           uint8, Pillow's 8-bit resampler
//   3. vertical pass, cropped output row y:
//        v(y, x) = clip8((2^21 + sum_j t(vb[y].start + j, x) * vk[y][j]) >> 22)
//   4. out[c][y][x] = (v / 255.f - mean[c]) / std[c]            fp32, two correctly rounded divisions (torchvision's sub_ / div_)
// The tables already hold the centre crop (entry x is resized column x + left).  An axis whose size does not change has the
// identity table (one tap of weight 2^22 at x + left): (2^21 + q * 2^22) >> 22 = q, the skipped pass bit for bit.
// Pass 2 writes an RGBX uint8 intermediate [n][H][n_px]; pass 3 reads it.  Indices into the source and the intermediate are
// clamped to the image, so a bad table gives wrong pixels, never an access outside the buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shapeclipper_hip.h"

namespace sc_clip_pre {

constexpr int THREADS = 256;
constexpr int MAX_SIDE = 16384;
constexpr int MAX_NPX = 2048;
constexpr int MAX_TAPS = 1024;
constexpr int PRECISION_BITS = 22;

__device__ __forceinline__ unsigned int clip8(int v) {
    v >>= PRECISION_BITS;                        // arithmetic shift
    return (unsigned int)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ void clamp_span(const int* bounds, int i, int taps, int size, int& start, int& count) {
    start = bounds[2 * i];
    count = bounds[2 * i + 1];
    start = start < 0 ? 0 : (start > size - 1 ? size - 1 : start);
    count = count < 0 ? 0 : count;
    count = count > taps ? taps : count;
    count = count > size - start ? size - start : count;
}

// grid: (ceil(n_px / THREADS), H, n) -- one thread per (image, source row, cropped output column), three channels
__global__ void __launch_bounds__(THREADS) horizontal(const uint32_t* __restrict__ rgba, int H, int W, int n_px, int bg,
                                                      const int* __restrict__ bounds, const int* __restrict__ coef, int taps,
                                                      uint32_t* __restrict__ tmp) {
    const int x = blockIdx.x * THREADS + threadIdx.x;
    if (x >= n_px) return;
    const int r = blockIdx.y;
    const size_t img = blockIdx.z;
    const uint32_t* row = rgba + (img * H + r) * (size_t)W;
    int start, count;
    clamp_span(bounds, x, taps, W, start, count);
    const int* k = coef + (size_t)x * taps;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int i = 0; i < count; ++i) {
        uint32_t p = row[start + i];
        const int w = k[i];
        if (bg >= 0 && (p >> 24) < 128u) p = (uint32_t)bg * 0x010101u;
        s0 += (int)(p & 0xFF) * w;
        s1 += (int)((p >> 8) & 0xFF) * w;
        s2 += (int)((p >> 16) & 0xFF) * w;
    }
    tmp[(img * H + r) * (size_t)n_px + x] = clip8(s0) | (clip8(s1) << 8) | (clip8(s2) << 16);
}

// grid: (ceil(n_px / THREADS), n_px, n) -- one thread per output pixel
__global__ void __launch_bounds__(THREADS) vertical(const uint32_t* __restrict__ tmp, int H, int n_px, const int* __restrict__ bounds,
                                                    const int* __restrict__ coef, int taps, float* __restrict__ out) {
    const int x = blockIdx.x * THREADS + threadIdx.x;
    if (x >= n_px) return;
    const int y = blockIdx.y;
    const size_t img = blockIdx.z;
    const uint32_t* col = tmp + img * H * (size_t)n_px + x;
    int start, count;
    clamp_span(bounds, y, taps, H, start, count);
    const int* k = coef + (size_t)y * taps;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < count; ++j) {
        const uint32_t p = col[(size_t)(start + j) * n_px];
        const int w = k[j];
        s0 += (int)(p & 0xFF) * w;
        s1 += (int)((p >> 8) & 0xFF) * w;
        s2 += (int)((p >> 16) & 0xFF) * w;
    }
    // openai/CLIP's Normalize constants, as fp32 (torchvision makes float32 tensors of them)
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
    const float stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    const unsigned int v[3] = {clip8(s0), clip8(s1), clip8(s2)};
    const size_t plane = (size_t)n_px * n_px;
    float* o = out + img * 3 * plane + (size_t)y * n_px + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = ((float)v[c] / 255.0f - mean[c]) / stdv[c];
}

}  // namespace sc_clip_pre

extern "C" int sc_clip_preprocess(const unsigned char* rgba, int n, int H, int W, int n_px, int bg, const int* h_bounds, const int* h_coef,
                                  int h_taps, const int* v_bounds, const int* v_coef, int v_taps, unsigned char* tmp, float* out,
                                  void* stream) {
    using namespace sc_clip_pre;
    if (n < 0 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || n_px < 1 || n_px > MAX_NPX || bg < -1 || bg > 255 ||
        h_taps < 1 || h_taps > MAX_TAPS || v_taps < 1 || v_taps > MAX_TAPS || n > 65535)
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!rgba || !h_bounds || !h_coef || !v_bounds || !v_coef || !tmp || !out) return (int)hipErrorInvalidValue;
    // pointers are read and written as 32-bit words
    if (((uintptr_t)rgba | (uintptr_t)tmp | (uintptr_t)out) & 3) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const unsigned int gx = (unsigned int)((n_px + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(horizontal, dim3(gx, (unsigned int)H, (unsigned int)n), dim3(THREADS), 0, s, (const uint32_t*)rgba, H, W, n_px, bg,
                       h_bounds, h_coef, h_taps, (uint32_t*)tmp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(vertical, dim3(gx, (unsigned int)n_px, (unsigned int)n), dim3(THREADS), 0, s, (const uint32_t*)tmp, H, n_px,
                       v_bounds, v_coef, v_taps, out);
    return (int)hipGetLastError();
}
