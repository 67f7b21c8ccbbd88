// block_scan.hpp -- the exclusive prefix sum of one value per thread over a wave and over a workgroup of WAVES full waves.
// Integer sums in a fixed association: the same bits whatever the launch.  (loss.hip, silhouette_rays.hip and rgb_common.hpp keep scans of
// their own: unsigned radix-select counts, an explicit width, floats.)
#pragma once
#include <hip/hip_runtime.h>

namespace sc_scan {

// inclusive prefix of v over the 64 lanes of the wave (lane 63 ends up holding the wave's total); every lane calls it
template <class T>
__device__ __forceinline__ T wave_inclusive(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// Exclusive prefix of v over the workgroup (threads in threadIdx.x order) and, in `total`, the sum over the workgroup.  Every thread of
// the WAVES * 64 calls it; wave_tot is LDS for WAVES values.  There is exactly ONE barrier inside, between the waves writing their totals
// and everybody reading them.  A caller that scans again with the same wave_tot must put a barrier of its own between the two calls (the
// emit loops of isosurface.hip and dual_contour.hip end their round with one anyway): the next round's totals would otherwise overwrite
// values a slower wave has not read yet.
template <int WAVES, class T>
__device__ __forceinline__ T block_exclusive(T v, T* wave_tot, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive(v);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const T t = wave_tot[w];
        if (w < wave) before += t;
        total += t;
    }
    return before + incl - v;
}

}  // namespace sc_scan
