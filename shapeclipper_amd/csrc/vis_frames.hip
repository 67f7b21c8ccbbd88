// vis_frames.hip -- uint8 RGB frames of the turn-table GIFs from the render chain's per-ray outputs, exactly as the reference builds them.
//
// Reference: model/runner.py:417-424 (vis_rotate: the [B,R,c] outputs viewed as [B,c,H,W] maps, normals / 2 + 0.5), then
// utils/util_vis.py:68-75 (dump_gifs) -> :35-44 (preprocess_vis_image) -> :77-80 (get_heatmap for one channel) and
// Image.fromarray((img * 255).astype(np.uint8)).  Per value x of a frame (all arithmetic fp32, this file is built without contraction):
//   RGB    : v = clamp((x - lo) * scale, 0, 1);  byte = trunc(v * 255)
//   normal : x' = x * 0.5 + 0.5 (torch's `/ 2` is a multiply by 0.5), then as RGB
//   mask   : v = clamp((x - lo) * scale, 0, 1);  i = trunc(v * 256), 256 -> 255;  byte = i on all three channels.  matplotlib's `gray`
//            colormap maps index i to float64 i / 255; the reference then goes float64 -> fp32 -> * 255 -> trunc, which gives i back
//            for every index (tests/golden/vis_gray_lut.npz holds the table).  Not the RGB formula: 0.5 gives 128 here, 127 there.
// scale = fp32 1 / (hi - lo): torch divides a device tensor by a Python number as a multiply by its fp32 reciprocal.
// NaN writes 0.  The reference's float -> uint8 cast is undefined for NaN RGB values; its mask path maps NaN to the colormap's
// "bad" colour (0, 0, 0), so 0 is what it writes there.
// The ray order of an image is row-major pixel order, so frame bytes are the per-ray values in order: no transpose.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shapeclipper_hip.h"

namespace sc_vis {

constexpr int THREADS = 256;
constexpr int BYTES_PER_THREAD = 4;           // one 32-bit store per thread
constexpr unsigned int MAX_BLOCKS = 65536;    // grid-stride beyond this

enum Kind { RGB = 0, MASK = 1, NORMAL = 2 };

__device__ __forceinline__ unsigned int rgb_byte(float x, float lo, float scale) {
    const float v = (x - lo) * scale;
    if (v != v) return 0u;                                    // NaN
    const float c = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    return (unsigned int)(c * 255.0f);                        // truncation, c * 255 in [0, 255]
}

__device__ __forceinline__ unsigned int mask_byte(float x, float lo, float scale) {
    const float v = (x - lo) * scale;
    if (v != v) return 0u;
    const float c = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    const unsigned int i = (unsigned int)(c * 256.0f);        // exact product (power of two), then truncation
    return i > 255u ? 255u : i;
}

// byte j of the frame buffer [n_pixels][3]: RGB / normal read x[j], mask reads x[j / 3]
template <int KIND>
__device__ __forceinline__ unsigned int frame_byte(const float* __restrict__ x, long long j, float lo, float scale) {
    if (KIND == MASK) return mask_byte(x[j / 3], lo, scale);
    float v = x[j];
    if (KIND == NORMAL) v = v * 0.5f + 0.5f;
    return rgb_byte(v, lo, scale);
}

template <int KIND>
__global__ void __launch_bounds__(THREADS) frames_kernel(const float* __restrict__ x, long long n_bytes, float lo, float scale,
                                                         uint8_t* __restrict__ out) {
    const long long stride = (long long)gridDim.x * THREADS * BYTES_PER_THREAD;
    for (long long j0 = ((long long)blockIdx.x * THREADS + threadIdx.x) * BYTES_PER_THREAD; j0 < n_bytes; j0 += stride) {
        if (j0 + BYTES_PER_THREAD <= n_bytes) {
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < BYTES_PER_THREAD; ++k) w |= frame_byte<KIND>(x, j0 + k, lo, scale) << (8 * k);
            *reinterpret_cast<uint32_t*>(out + j0) = w;       // out is 4-byte aligned and j0 a multiple of 4
        } else {
            for (long long j = j0; j < n_bytes; ++j) out[j] = (uint8_t)frame_byte<KIND>(x, j, lo, scale);
        }
    }
}

}  // namespace sc_vis

extern "C" int sc_vis_frames(const float* x, long long n_pixels, int channels, int kind, float lo, float scale, unsigned char* out,
                             void* stream) {
    using namespace sc_vis;
    if (n_pixels < 0 || n_pixels > (1LL << 40)) return (int)hipErrorInvalidValue;
    if (!((kind == RGB && channels == 3) || (kind == NORMAL && channels == 3) || (kind == MASK && channels == 1)))
        return (int)hipErrorInvalidValue;
    if (n_pixels == 0) return 0;
    if (!x || !out || ((uintptr_t)out & 3)) return (int)hipErrorInvalidValue;
    const long long n_bytes = n_pixels * 3;
    const long long per_block = (long long)THREADS * BYTES_PER_THREAD;
    long long blocks = (n_bytes + per_block - 1) / per_block;
    if (blocks > (long long)MAX_BLOCKS) blocks = MAX_BLOCKS;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned int)blocks), block(THREADS);
    if (kind == RGB)
        hipLaunchKernelGGL(frames_kernel<RGB>, grid, block, 0, s, x, n_bytes, lo, scale, (uint8_t*)out);
    else if (kind == NORMAL)
        hipLaunchKernelGGL(frames_kernel<NORMAL>, grid, block, 0, s, x, n_bytes, lo, scale, (uint8_t*)out);
    else
        hipLaunchKernelGGL(frames_kernel<MASK>, grid, block, 0, s, x, n_bytes, lo, scale, (uint8_t*)out);
    return (int)hipGetLastError();
}
