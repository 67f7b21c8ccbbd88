// surface_hit.hip -- the per-ray root finder of the surface render (`--hip.surface_render`, Renderer.render_surface).
//
//   sc_ray_first_crossing : the first outside -> inside sign change of sdf - iso along each ray's S samples (one 64-lane wave per ray,
//                           S walked in chunks of 64, one ballot per chunk, no atomics) -> the bracket [t_lo, t_hi] and its two values
//   sc_ray_bracket_step   : one lane per ray: take the SDF value at the previous query into the bracket, then the next query by regula
//                           falsi with a bisection safeguard, and the point cam_loc + t * ray_dir of that query
//
// include/shapeclipper_hip.h states both algorithms exactly; tests/surface_hit_ref.py restates them in numpy, and the GPU tests compare
// bits.  Every fp32 operation below is a single rounding (no contraction: the Makefile compiles this file with -ffp-contract=off and the
// kernels carry the pragma as render.hip does), comparisons are true comparisons (a NaN fails them all).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/shapeclipper_hip.h"

namespace sc {

// lane == sample 64 c + lane of chunk c; 4 rays per workgroup
__global__ __launch_bounds__(256) void ray_first_crossing_kernel(const float* __restrict__ z_vals, const float* __restrict__ sdf, int n_rays,
                                                                 int S, float iso, float* __restrict__ t_lo, float* __restrict__ t_hi,
                                                                 float* __restrict__ f_lo, float* __restrict__ f_hi,
                                                                 int32_t* __restrict__ hit) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    for (int ray = blockIdx.x * 4 + (threadIdx.x >> 6); ray < n_rays; ray += gridDim.x * 4) {
        const size_t base = (size_t)ray * S;
        const float f0 = __fsub_rn(sdf[base], iso);             // the same address in every lane: one broadcast load
        int found = -1;                                          // wave-uniform: the sample index i of the bracket (i, i + 1)
        float fi = f0, fn = f0;
        if (!(f0 <= 0.0f)) {                                     // (a NaN at sample 0 is not "inside": the ray is searched)
            for (int c = 0; c < S && found < 0; c += 64) {
                const int i = c + lane;
                fi = i < S ? __fsub_rn(sdf[base + i], iso) : __int_as_float(0x7fc00000);
                fn = __shfl_down(fi, 1);
                if (lane == 63)                                  // the pair that straddles two chunks: sample 64 (c + 1) is the next chunk's
                    fn = i + 1 < S ? __fsub_rn(sdf[base + i + 1], iso) : __int_as_float(0x7fc00000);
                // lanes past S hold NaN, so neither (S - 1, S) nor anything later forms a bracket
                const unsigned long long m = __ballot(fi > 0.0f && fn <= 0.0f);
                if (m) found = c + __ffsll((long long)m) - 1;    // the smallest i of this chunk; earlier chunks had none
            }
        }
        if (found >= 0) {
            if (lane == (found & 63)) {
                t_lo[ray] = z_vals[base + found];
                t_hi[ray] = z_vals[base + found + 1];
                f_lo[ray] = fi;
                f_hi[ray] = fn;
                hit[ray] = 1;
            }
        } else if (lane == 0) {
            const float z0 = z_vals[base];
            t_lo[ray] = z0;
            t_hi[ray] = z0;
            f_lo[ray] = f0;
            f_hi[ray] = f0;
            hit[ray] = f0 <= 0.0f ? 2 : 0;
        }
    }
}

// lane == ray.  t_prev may be t, and the bracket is updated in place: a lane reads all it needs of its ray before it writes
__global__ __launch_bounds__(256) void ray_bracket_step_kernel(const float* __restrict__ cam_loc, const float* __restrict__ ray_dirs,
                                                               const float* __restrict__ f_new, const float* t_prev, int n_rays, float iso,
                                                               float* __restrict__ t_lo, float* __restrict__ t_hi, float* __restrict__ f_lo,
                                                               float* __restrict__ f_hi, const int32_t* __restrict__ hit, float* t,
                                                               float* __restrict__ points) {
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t ray = (size_t)blockIdx.x * 256 + threadIdx.x; ray < (size_t)n_rays; ray += stride) {
        float lo = t_lo[ray], hi = t_hi[ray], flo = f_lo[ray], fhi = f_hi[ray];
        float q = lo;
        if (hit[ray] == 1) {
            if (f_new) {
                const float f = __fsub_rn(f_new[ray], iso), tp = t_prev[ray];
                if (f > 0.0f) {
                    lo = tp; flo = f;
                    t_lo[ray] = lo; f_lo[ray] = flo;
                } else if (f <= 0.0f) {
                    hi = tp; fhi = f;
                    t_hi[ray] = hi; f_hi[ray] = fhi;
                }                                               // NaN: the bracket stays
            }
            const float d = __fsub_rn(flo, fhi);
            float w = __fdiv_rn(flo, d);
            if (!(d <= 3.402823466e+38f) || !(w >= 0.0f && w <= 1.0f)) w = 0.5f;   // d overflowed or is NaN, or w is: bisect
            q = __fadd_rn(lo, __fmul_rn(w, __fsub_rn(hi, lo)));
            if (!(q >= lo)) q = lo;
            if (!(q <= hi)) q = hi;
        }
        t[ray] = q;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            points[ray * 3 + k] = __fadd_rn(cam_loc[ray * 3 + k], __fmul_rn(q, ray_dirs[ray * 3 + k]));      // the ray sampler's expression
    }
}

}  // namespace sc

extern "C" {

int sc_ray_first_crossing(const float* z_vals, const float* sdf, int n_rays, int n_samples, float iso, float* t_lo, float* t_hi,
                          float* f_lo, float* f_hi, int32_t* hit, void* stream_) {
    if (!SC_N_SAMPLES_SUPPORTED(n_samples)) return (int)hipErrorInvalidValue;
    if (n_rays <= 0) return 0;
    if (n_rays > SC_SURFACE_HIT_MAX_RAYS || !z_vals || !sdf || !t_lo || !t_hi || !f_lo || !f_hi || !hit) return (int)hipErrorInvalidValue;
    int blocks = (n_rays + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(sc::ray_first_crossing_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, z_vals, sdf, n_rays, n_samples,
                       iso, t_lo, t_hi, f_lo, f_hi, hit);
    return (int)hipGetLastError();
}

int sc_ray_bracket_step(const float* cam_loc, const float* ray_dirs, const float* f_new, const float* t_prev, int n_rays, float iso,
                        float* t_lo, float* t_hi, float* f_lo, float* f_hi, const int32_t* hit, float* t, float* points, void* stream_) {
    if (n_rays <= 0) return 0;
    if (n_rays > SC_SURFACE_HIT_MAX_RAYS || !cam_loc || !ray_dirs || !t_lo || !t_hi || !f_lo || !f_hi || !hit || !t || !points || (f_new && !t_prev))
        return (int)hipErrorInvalidValue;
    int blocks = (n_rays + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(sc::ray_bracket_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, cam_loc, ray_dirs, f_new, t_prev,
                       n_rays, iso, t_lo, t_hi, f_lo, f_hi, hit, t, points);
    return (int)hipGetLastError();
}

}  // extern "C"
