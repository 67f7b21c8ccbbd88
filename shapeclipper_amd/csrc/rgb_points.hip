// rgb_points.hip -- the RGB network at arbitrary points (mesh vertices), plus the unit normal of the SDF there.
//
// RGBNetwork.forward (model/implicit.py:220-239) without the rays: consumes what sdf_fwd / sdf_fwd_stream left in HBM for the points
// (d sdf/dx, 64-channel feature in TBL64 layout) and writes one sigmoid colour and one unit normal grad / max(|grad|, 1e-12) per point.
// The chain is that of rgb_composite_fwd_split_kernel (rgb_fwd.hip): the same pre-split bf16x3 fragments in LDS (rgb_presplit.hpp), the
// same staging, product parts, ReLU / split and output layer, so a point's colour is bit-identical to its rgb_flat entry in a render.
// One wave walks 16-point tiles two at a time (a weight fragment read feeds both); density, compositing and parked activations are not
// here.  The image of a tile is tile * 16 / n_per_image, as in the SDF kernels, so n_per_image is a multiple of 16.  The last tile may
// hold fewer than 16 points: lanes past n_points load nothing (zeros enter the chain in their own MFMA columns) and store nothing.
#include "../../include/shapeclipper_hip.h"
#include "rgb_presplit.hpp"

namespace sc {

struct RgbPointsArgs {
    const float* points;   // [n_points][3]
    const float* grad;     // [n_points][3]   d sdf / d point (read when normal is given)
    const float* feat;     // TBL64, ceil(n_points / 16) tiles (read when rgb is given)
    const float* v;        // RgbPack image
    const float* dbias;    // [n_images][3][64]
    int n_points, n_per_image, n_images, symmetric;
    float* rgb;            // [n_points][3] or null
    float* normal;         // [n_points][3] or null
};

__global__ __launch_bounds__(64 * rs::WAVES) void rgb_points_kernel(RgbPointsArgs a) {
    using namespace rs;
    extern __shared__ __attribute__((aligned(16))) char lds_c[];
    if (a.rgb) {                                                         // uniform over the launch
        stage_weights(lds_c, a.v, threadIdx.x, 64 * WAVES);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = lane & 15, g = lane >> 4;
    const float* v3 = reinterpret_cast<const float*>(lds_c + OFF_V3) + 4 * g;
    const float* b3 = reinterpret_cast<const float*>(lds_c + OFF_V3) + 3 * 64;
    const int n_tiles = (a.n_points + TP - 1) / TP, n_pairs = (n_tiles + 1) >> 1;

    for (int pair = blockIdx.x * WAVES + wave; pair < n_pairs; pair += gridDim.x * WAVES) {
        size_t pt[2];
        bool valid[2];
        const float* db[2];
        float x0[2], x1[2], x2[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int tile = 2 * pair + u;
            pt[u] = (size_t)tile * TP + p;
            valid[u] = pt[u] < (size_t)a.n_points;
            const int img = min((int)((size_t)tile * TP / a.n_per_image), a.n_images - 1);
            db[u] = a.dbias + (size_t)img * 192 + 4 * g;
            x0[u] = valid[u] ? a.points[pt[u] * 3 + 0] : 0.f;
            x1[u] = valid[u] ? a.points[pt[u] * 3 + 1] : 0.f;
            x2[u] = valid[u] ? a.points[pt[u] * 3 + 2] : 0.f;
        }
        if (a.normal && g == 1) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (!valid[u]) continue;
                const float gx = a.grad[pt[u] * 3 + 0], gy = a.grad[pt[u] * 3 + 1], gz = a.grad[pt[u] * 3 + 2];
                const float inv = 1.f / fmaxf(sqrtf(gx * gx + gy * gy + gz * gz), 1e-12f);
                a.normal[pt[u] * 3 + 0] = gx * inv;
                a.normal[pt[u] * 3 + 1] = gy * inv;
                a.normal[pt[u] * 3 + 2] = gz * inv;
            }
        }
        if (!a.rgb) continue;
        MlpPieces<8> e32[2], fp[2][2], hp[2][2];
        MlpPieces<4> e16[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float f[ACT_STEPS] = {};
            if (valid[u]) tbl_load(a.feat, 2 * pair + u, p, g, f);
            float e[PE_STEPS], d1[PE_STEPS], d2[PE_STEPS];
            pe_slots<false, false>(x0[u], x1[u], x2[u], g, a.symmetric != 0, e, d1, d2);
            split_pe(e, e32[u], e16[u]);
            split_act(f, fp[u]);
        }
        f32x4 acc[2][NT];
        float r[2][ACT_STEPS];
        // layer l: acc = bias; products; r = relu(acc); split for the next layer (the order of rgb_composite_fwd_split_kernel)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc_init(acc[u], db[u]);
        hidden_part<2>(lds_c + OFF_V0F, lane, fp, acc);
        pe_part<2>(lds_c + OFF_V0E, lane, e32, e16, acc);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            relu_from_acc(acc[u], r[u]);
            split_act(r[u], hp[u]);
            acc_init(acc[u], db[u] + 64);
        }
        hidden_part<2>(lds_c + OFF_V1, lane, hp, acc);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            relu_from_acc(acc[u], r[u]);
            split_act(r[u], hp[u]);
            acc_init(acc[u], db[u] + 128);
        }
        hidden_part<2>(lds_c + OFF_V2, lane, hp, acc);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            relu_from_acc(acc[u], r[u]);
            float col[3];
            head(v3, b3, r[u], col);
            if (g == 0 && valid[u]) {
                a.rgb[pt[u] * 3 + 0] = col[0];
                a.rgb[pt[u] * 3 + 1] = col[1];
                a.rgb[pt[u] * 3 + 2] = col[2];
            }
        }
    }
}

}  // namespace sc

extern "C" int sc_rgb_points_forward_split(const float* points, const float* grad, const float* feat, const float* v_pack,
                                           const float* dbias, int n_points, int n_per_image, int n_images, int symmetric,
                                           float* rgb, float* normal, void* stream_) {
    if (n_points < 0 || n_per_image <= 0 || n_per_image % sc::TP != 0 || n_images <= 0) return (int)hipErrorInvalidValue;
    if (n_points == 0 || (!rgb && !normal)) return 0;
    const sc::RgbPointsArgs a{points, grad, feat, v_pack, dbias, n_points, n_per_image, n_images, symmetric, rgb, normal};
    const int n_pairs = ((n_points + sc::TP - 1) / sc::TP + 1) / 2;
    int blocks = (n_pairs + sc::rs::WAVES - 1) / sc::rs::WAVES;
    if (blocks > 256) blocks = 256;   // one 8-wave workgroup per CU (90 KiB of pre-split fragments)
    (void)hipFuncSetAttribute((const void*)sc::rgb_points_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, sc::rs::LDS_BYTES);
    hipLaunchKernelGGL(sc::rgb_points_kernel, dim3(blocks), dim3(64 * sc::rs::WAVES), sc::rs::LDS_BYTES, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}
