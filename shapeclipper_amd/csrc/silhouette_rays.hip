// silhouette_rays.hip -- importance ray choice of the Pix3D training loader on the device.
//
// Reference: data/pix3d.py:230-239 calls utils/util.py:237-248 (compute_sampling_prob) once per view: a boundary distance
// transform of the mask (vigra boundaryDistanceTransform), weights w = 1 / (d + uniform_fac), then
// np.random.choice(H*W, n_rays, replace=False, p=w / sum w).  Here both halves run over a batch of masks, one workgroup per mask.
//
// sc_silhouette_distance: a pixel is inside when mask > 0.5.  d = |p - q| - 0.5 with q the centre of the nearest pixel of the
// other class (the image border is not a boundary), computed in exact integer squared distances n = dx^2 + dy^2:
//   1. the mask goes to LDS as one bit per pixel (rows of 64-bit words, built with a wave ballot);
//   2. for a strip of columns, h(y, x) = horizontal distance from (y, x) to the nearest pixel of the OTHER class in row y
//      (bit scans over the row's words), 16 bits per pixel in LDS;
//   3. column pass: n(y, x) = min over rows y' of (y - y')^2 + g(y', x)^2, with g = 0 where (y', x) itself is of the other class of
//      (y, x) and h(y', x) otherwise, searched outwards from y and stopped once (y - y')^2 >= the best n;
//   4. d = float(sqrt_rn(double(n)) - 0.5): the double square root is checked against the two neighbouring rounding midpoints in
//      exact 128-bit integer arithmetic, so the result is the correctly rounded one whatever the device square root gives; the
//      subtraction of 0.5 is exact and the conversion to float rounds to nearest even (numpy's float32(sqrt(float64(n)) - 0.5)).
//   A mask of a single class has no boundary: every pixel gets d = 0 (a uniform draw).
//
// sc_silhouette_rays: weighted draw without replacement as an exponential race.  Pixel i of mask m gets the key
//   key_i = -log(u_i) * (double(d_i) + uniform_fac)          (double precision; a key that is NaN or negative is replaced by NaN)
// and the n_rays smallest keys in increasing order are the draw (ties to the lower pixel index): the ordered result has the law
// of successive sampling, i.e. of np.random.choice(replace=False, p ~ w).  The uniforms come from a counter hash of the mask's seed:
//   fmix(z) = splitmix64's finaliser:  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
//   base = fmix(uint64(seed)),  z_i = fmix(base + (i + 1) * 0x9E3779B97F4A7C15)   (mod 2^64)
//   u_i = ((z_i >> 11) + 1) * 2^-53                                               in (0, 1]
// so a mask's draw depends on its seed, its distances and n_rays only.  Selection: the keys (a pure function of seed, pixel and
// d) are recomputed in each pass instead of being held -- 50,176 doubles per 224x224 mask do not fit in LDS.  The composite
// c = (key bits without the sign) << 20 | pixel (83 bits; positive doubles order like their bit patterns, and c is unique) is
// radix-selected with 12-bit LDS histograms, most significant digit first, until the candidates at or below the cut fit the LDS
// buffer; those are collected, bitonic-sorted in LDS and written in order.  Ranks are settled in rounds of up to CHUNK, so that
// n_rays up to H*W (a permutation) works with the same buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shapeclipper_hip.h"

namespace sc_sil {

constexpr int THREADS = 1024;
constexpr int MAX_SIDE = 512;
constexpr int MAX_WORDS = MAX_SIDE / 64;                 // 64-bit words per bit row
constexpr int STRIP_PIXELS = 16384;                      // h values held in LDS per column strip (32 KiB)
constexpr unsigned short H_NONE = 0xFFFF;                // no pixel of the other class in the row
constexpr unsigned int N_NONE = 0xFFFFFFFFu;

constexpr int DIGIT_BITS = 12;
constexpr int NBIN = 1 << DIGIT_BITS;
constexpr int COMP_BITS = 83;                            // 63 key bits + 20 index bits
constexpr int IDX_BITS = 20;
constexpr int CAP = 4096;                                // candidate buffer (pairs) in LDS
constexpr int CHUNK = 2048;                              // ranks settled per round (<= CAP)

typedef unsigned __int128 u128;

// ------------------------------------------------------------------------------------------------------------------------
// distance

// exact: sign of (a * 2^s - b^2) for a * 2^s, b^2 < 2^128
__device__ __forceinline__ int cmp_scaled(u128 a_scaled, u128 b) {
    const u128 b2 = b * b;
    return a_scaled < b2 ? -1 : (a_scaled > b2 ? 1 : 0);
}

// float(sqrt_rn(double(n)) - 0.5) for 1 <= n < 2^20
__device__ float boundary_value(unsigned int n) {
    double s = sqrt((double)n);
    // s = M * 2^e, 2^52 <= M < 2^53.  The midpoints next to s are (4M +- 2) * 2^(e-2) (4M - 1 below a power of two).  s is the
    // correctly rounded root iff  lo_mid^2 <= n <= hi_mid^2  (sqrt of a non-square integer is irrational: no ties).  Compare
    // n * 2^(4 - 2e) with (4M +- .)^2 exactly; 4 - 2e <= 108 and n * 2^(4-2e) ~ 16 M^2 < 2^111.
    for (int it = 0; it < 2; ++it) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(s);
        const int e = (int)((bits >> 52) & 0x7FF) - 1075;
        const unsigned long long M = (bits & 0xFFFFFFFFFFFFFull) | (1ull << 52);
        const u128 scaled = (u128)n << (4 - 2 * e);
        const u128 hi_mid = (u128)(4 * M + 2);
        const u128 lo_mid = (u128)(M == (1ull << 52) ? 4 * M - 1 : 4 * M - 2);
        if (cmp_scaled(scaled, hi_mid) > 0) {
            s = __longlong_as_double((long long)(bits + 1));
        } else if (cmp_scaled(scaled, lo_mid) < 0) {
            s = __longlong_as_double((long long)(bits - 1));
        } else {
            break;
        }
    }
    return (float)(s - 0.5);
}

__device__ __forceinline__ int bit_at(const unsigned long long* rows, int words, int y, int x) {
    return (int)((rows[y * words + (x >> 6)] >> (x & 63)) & 1ull);
}

// horizontal distance from (y, x) to the nearest pixel of the other class in row y, H_NONE if there is none
__device__ unsigned short row_distance(const unsigned long long* rows, int words, int W, int y, int x) {
    const unsigned long long* r = rows + y * words;
    const int c = (int)((r[x >> 6] >> (x & 63)) & 1ull);
    const int k0 = x >> 6;
    int best = 0x7FFFFFFF;
    // right (the bit of x itself is of its own class: never set in `diff`)
    for (int k = k0; k < words; ++k) {
        unsigned long long diff = c ? ~r[k] : r[k];
        const int valid = W - k * 64;
        if (valid < 64) diff &= (1ull << valid) - 1ull;
        if (k == k0) diff &= ~0ull << (x & 63);
        if (diff) {
            best = k * 64 + __builtin_ctzll(diff) - x;
            break;
        }
    }
    for (int k = k0; k >= 0; --k) {
        unsigned long long diff = c ? ~r[k] : r[k];
        const int valid = W - k * 64;
        if (valid < 64) diff &= (1ull << valid) - 1ull;
        if (k == k0) diff &= (x & 63) == 63 ? ~0ull : ((2ull << (x & 63)) - 1ull);
        if (diff) {
            const int d = x - (k * 64 + 63 - __builtin_clzll(diff));
            best = d < best ? d : best;
            break;
        }
    }
    return best == 0x7FFFFFFF ? H_NONE : (unsigned short)best;
}

__global__ void __launch_bounds__(THREADS) silhouette_distance_kernel(const float* __restrict__ masks, int H, int W,
                                                                       float* __restrict__ dist) {
    __shared__ unsigned long long rows[MAX_SIDE * MAX_WORDS];
    __shared__ unsigned short hbuf[STRIP_PIXELS];
    __shared__ int any_other;
    const long long P = (long long)H * W;
    const float* m = masks + (long long)blockIdx.x * P;
    float* out = dist + (long long)blockIdx.x * P;
    const int words = (W + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = THREADS / 64;
    if (threadIdx.x == 0) any_other = 0;
    // 1. bit rows: one wave per 64-pixel word
    for (int w = wave; w < H * words; w += nwaves) {
        const int y = w / words, x = (w - y * words) * 64 + lane;
        const bool in = x < W && m[(long long)y * W + x] > 0.5f;
        const unsigned long long b = __ballot(in);
        if (lane == 0) rows[w] = b;
    }
    __syncthreads();
    // single-class mask?  (both classes present iff some row word differs from all-0 / all-1 of the first pixel's class)
    {
        const int c0 = (int)(rows[0] & 1ull);
        int differs = 0;
        for (int w = threadIdx.x; w < H * words; w += THREADS) {
            const int valid = W - (w % words) * 64;
            const unsigned long long vm = valid < 64 ? (1ull << valid) - 1ull : ~0ull;
            const unsigned long long want = c0 ? vm : 0ull;
            differs |= (rows[w] & vm) != want;
        }
        if (differs) any_other = 1;        // benign race: every writer stores 1
    }
    __syncthreads();
    if (!any_other) {
        for (long long p = threadIdx.x; p < P; p += THREADS) out[p] = 0.0f;
        return;
    }
    const int strip = STRIP_PIXELS / H < W ? STRIP_PIXELS / H : W;      // columns per strip (H <= 512: >= 32)
    for (int x0 = 0; x0 < W; x0 += strip) {
        const int sw = W - x0 < strip ? W - x0 : strip;
        // 2. row distances of the strip
        for (int p = threadIdx.x; p < H * sw; p += THREADS) {
            const int y = p / sw, x = x0 + (p - y * sw);
            hbuf[p] = row_distance(rows, words, W, y, x);
        }
        __syncthreads();
        // 3. column pass + 4. value
        for (int p = threadIdx.x; p < H * sw; p += THREADS) {
            const int y = p / sw, xs = p - y * sw, x = x0 + xs;
            const int c = bit_at(rows, words, y, x);
            unsigned int best = N_NONE;
            for (int dy = 0; dy < H; ++dy) {
                const unsigned int dy2 = (unsigned int)(dy * dy);
                if (dy2 >= best) break;
                for (int side = 0; side < (dy ? 2 : 1); ++side) {
                    const int yy = side ? y + dy : y - dy;
                    if (yy < 0 || yy >= H) continue;
                    unsigned int g;
                    if (bit_at(rows, words, yy, x) != c) {
                        g = 0;
                    } else {
                        const unsigned short h = hbuf[yy * sw + xs];
                        if (h == H_NONE) continue;
                        g = h;
                    }
                    const unsigned int cand = dy2 + g * g;
                    best = cand < best ? cand : best;
                }
            }
            out[(long long)y * W + x] = boundary_value(best);    // both classes exist: best is finite (>= 1)
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// draw

__device__ __forceinline__ unsigned long long fmix64(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ u128 composite(const float* d, unsigned long long base, double fac, int i) {
    const unsigned long long z = fmix64(base + (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull);
    const double u = (double)((z >> 11) + 1ull) * 0x1p-53;
    const double key = -log(u) * ((double)d[i] + fac);
    // -0.0 (u == 1) becomes +0.0; NaN / negative keys go last as a canonical NaN
    const unsigned long long kb = key >= 0.0 ? ((unsigned long long)__double_as_longlong(key) & 0x7FFFFFFFFFFFFFFFull)
                                             : 0x7FF8000000000000ull;
    return ((u128)kb << IDX_BITS) | (u128)(unsigned int)i;
}

// block-wide exclusive scan of one int per thread; returns the exclusive prefix, *total the sum
__device__ int block_exclusive_scan(int v, int* wave_sums, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
        const int s = wave_sums[w];
        before += w < wave ? s : 0;
        all += s;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

__global__ void __launch_bounds__(THREADS) silhouette_rays_kernel(const float* __restrict__ dist, int P, int n_rays, double fac,
                                                                   const long long* __restrict__ seeds, long long* __restrict__ ray_idx) {
    __shared__ unsigned int hist[NBIN];
    __shared__ unsigned long long ckey[CAP];
    __shared__ unsigned int cidx[CAP];
    __shared__ int wave_sums[THREADS / 64];
    __shared__ int s_digit, s_below_bin, s_count;
    const float* d = dist + (long long)blockIdx.x * P;
    long long* out = ray_idx + (long long)blockIdx.x * n_rays;
    const unsigned long long base = fmix64((unsigned long long)seeds[blockIdx.x]);
    const int bins_per_thread = NBIN / THREADS;

    bool have_prev = false;
    u128 prev = 0;                                        // composite of the last element written (rank lo - 1)
    for (int lo = 0; lo < n_rays;) {
        const int hi = n_rays - lo < CHUNK ? n_rays : lo + CHUNK;
        const int k = hi - 1;                             // global rank of this round's cut
        u128 prefix = 0;
        int below = 0, eq = 0, shift = COMP_BITS;
        // radix select: narrow the cut's prefix until the candidates (c > prev, c >> shift <= prefix) fit CAP
        while (true) {
            const int width = shift >= DIGIT_BITS ? DIGIT_BITS : shift;
            const int sh = shift - width;
            const unsigned int nb = 1u << width;
            for (int b = threadIdx.x; b < NBIN; b += THREADS) hist[b] = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < P; i += THREADS) {
                const u128 c = composite(d, base, fac, i);
                if ((c >> shift) == prefix) atomicAdd(&hist[(unsigned int)(c >> sh) & (nb - 1)], 1u);
            }
            __syncthreads();
            int local = 0;
            for (int j = 0; j < bins_per_thread; ++j) local += (int)hist[threadIdx.x * bins_per_thread + j];
            int total;
            const int excl = block_exclusive_scan(local, wave_sums, &total);
            // the bin holding rank k - below (within this prefix)
            const int want = k - below;
            if (want >= excl && want < excl + local) {
                int run = excl;
                for (int j = 0; j < bins_per_thread; ++j) {
                    const int b = threadIdx.x * bins_per_thread + j;
                    const int h = (int)hist[b];
                    if (want < run + h) {
                        s_digit = b;
                        s_below_bin = run;
                        break;
                    }
                    run += h;
                }
            }
            __syncthreads();
            const int v = s_digit;
            below += s_below_bin;
            eq = (int)hist[v];
            prefix = (prefix << width) | (u128)(unsigned int)v;
            shift = sh;
            __syncthreads();                               // hist is cleared by the next level
            if (below + eq - lo <= CAP || shift == 0) break;   // the first is always true once shift == 0 (eq == 1)
        }
        // collect the candidates
        if (threadIdx.x == 0) s_count = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < P; i += THREADS) {
            const u128 c = composite(d, base, fac, i);
            if ((c >> shift) <= prefix && (!have_prev || c > prev)) {
                const int pos = atomicAdd(&s_count, 1);
                if (pos < CAP) {                           // cnt == below + eq - lo <= CAP: never false
                    ckey[pos] = (unsigned long long)(c >> IDX_BITS);
                    cidx[pos] = (unsigned int)i;
                }
            }
        }
        __syncthreads();
        const int cnt = s_count;                           // == below + eq - lo <= CAP
        int n2 = 1;
        while (n2 < cnt) n2 <<= 1;
        for (int p = cnt + threadIdx.x; p < n2; p += THREADS) {
            ckey[p] = ~0ull;
            cidx[p] = ~0u;
        }
        __syncthreads();
        // bitonic sort of (key, index), ascending
        for (int size = 2; size <= n2; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = threadIdx.x; t < (n2 >> 1); t += THREADS) {
                    const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                    const bool up = (i & size) == 0;
                    const unsigned long long ki = ckey[i], kj = ckey[j];
                    const unsigned int ii = cidx[i], ij = cidx[j];
                    const bool gt = ki > kj || (ki == kj && ii > ij);
                    if (gt == up) {
                        ckey[i] = kj; ckey[j] = ki;
                        cidx[i] = ij; cidx[j] = ii;
                    }
                }
                __syncthreads();
            }
        }
        for (int j = threadIdx.x; j < hi - lo; j += THREADS) out[lo + j] = (long long)cidx[j];
        prev = ((u128)ckey[hi - lo - 1] << IDX_BITS) | (u128)cidx[hi - lo - 1];
        have_prev = true;
        lo = hi;
        __syncthreads();                                   // ckey / cidx are rewritten by the next round
    }
}

}  // namespace sc_sil

extern "C" int sc_silhouette_distance(const float* masks, int n, int H, int W, float* dist, void* stream) {
    if (n < 0 || H < 1 || W < 1 || H > sc_sil::MAX_SIDE || W > sc_sil::MAX_SIDE) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    hipLaunchKernelGGL(sc_sil::silhouette_distance_kernel, dim3(n), dim3(sc_sil::THREADS), 0, (hipStream_t)stream, masks, H, W, dist);
    return (int)hipGetLastError();
}

extern "C" int sc_silhouette_rays(const float* dist, int n, int H, int W, int n_rays, double uniform_fac, const long long* seeds,
                                  long long* ray_idx, void* stream) {
    if (n < 0 || H < 1 || W < 1 || H > sc_sil::MAX_SIDE || W > sc_sil::MAX_SIDE) return (int)hipErrorInvalidValue;
    if (n_rays < 1 || n_rays > H * W) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    hipLaunchKernelGGL(sc_sil::silhouette_rays_kernel, dim3(n), dim3(sc_sil::THREADS), 0, (hipStream_t)stream, dist, H * W, n_rays,
                       uniform_fac, seeds, ray_idx);
    return (int)hipGetLastError();
}
