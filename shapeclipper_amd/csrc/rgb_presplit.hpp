// rgb_presplit.hpp -- LDS image of the RGB network's pre-split bf16x3 weight fragments (namespace rs), shared by the two kernels that run
// the RGB chain in the exact three-piece split arithmetic: rgb_composite_fwd_split_kernel (rgb_fwd.hip: along rays, with the compositing)
// and rgb_points_kernel (rgb_points.hip: at arbitrary points, e.g. mesh vertices).
// 90 KiB of fragments ([V0 feature | V0 encoding | V1 | V2] + the fp32 output layer), so ONE 8-wave workgroup per CU.
#pragma once
#include "mlp_presplit.hpp"
#include "rgb_common.hpp"

namespace sc {
namespace rs {
using namespace ps;
constexpr int WAVES = 8;
constexpr int OFF_V0F = 0;                         // [ks][mt]: feature columns 48..111 of V0
constexpr int OFF_V0E = OFF_V0F + HID_BYTES;       // [mt]: encoding columns 0..47 of V0
constexpr int OFF_V1 = OFF_V0E + PE_BYTES;
constexpr int OFF_V2 = OFF_V1 + HID_BYTES;
constexpr int OFF_V3 = OFF_V2 + HID_BYTES;         // fp32: [3][64] + b3[3] (+1 pad)
constexpr int LDS_BYTES = OFF_V3 + (3 * 64 + 4) * 4;

// the whole image from the RgbPack weights (all threads of the workgroup; the caller synchronises)
__device__ __forceinline__ void stage_weights(char* lds, const float* __restrict__ v, int tid, int nt) {
    stage_hidden(lds + OFF_V0F, v + RgbPack::V0, 112, 48, tid, nt);
    stage_pe(lds + OFF_V0E, v + RgbPack::V0, 112, 0, tid, nt);
    stage_hidden(lds + OFF_V1, v + RgbPack::V1, 64, 0, tid, nt);
    stage_hidden(lds + OFF_V2, v + RgbPack::V2, 64, 0, tid, nt);
    float* v3 = reinterpret_cast<float*>(lds + OFF_V3);
    if (tid < 3 * 64 + 3) v3[tid] = v[RgbPack::V3 + tid];         // V3 [3][64] and b3 [3] are contiguous in the pack
}

// the fp32 output layer and the sigmoid of one point from the last hidden layer's activations r (v3 = the image's V3 + 4 g, b3 its bias);
// col is identical in the four lane groups of the point
__device__ __forceinline__ void head(const float* v3, const float* b3, const float (&r)[ACT_STEPS], float (&col)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float part = 0.f;
#pragma unroll
        for (int q = 0; q < ACT_STEPS; ++q) part = __builtin_fmaf(v3[j * 64 + kp(q)], r[q], part);
        const float yv = group_sum(part) + b3[j];
        col[j] = 1.f / (1.f + expf(-yv));
    }
}
}  // namespace rs
}  // namespace sc
