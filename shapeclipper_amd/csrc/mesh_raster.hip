// mesh_raster.hip -- triangle rasteriser of the indexed marching-cubes mesh: nearest face, camera depth and perspective-correct
// barycentrics per pixel centre, for every (image, view) of a call (eval_3D.mesh_render, `--eval.mesh_render`).
//
// include/shapeclipper_hip.h states every expression operation by operation; tests/mesh_raster_ref.py restates them in numpy and the
// GPU tests compare bit for bit, so this file is built without contraction (Makefile) and keeps the stated order.  Coverage is integer
// arithmetic on a 1/256-pixel lattice (int64 edge functions, top-left rule); visibility is a 64-bit integer atomicMin on
// (bits(depth) << 32) | face, the key form of point_mesh.hip; nothing else is atomic but integer counters, so the outputs are the same
// bits from run to run.
//
// Launches: memsets (keys, list cursors, stats), project (a thread per (view, vertex): every vertex is projected once per view, not
// once per face that uses it), faces (a thread per (image, view, face): cull, count, rasterise a small face or list a large one), wave
// (a wave per listed face, lanes striding over its box), resolve (a thread per pixel).  Both coverage paths go through shade(), so
// they cannot disagree.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shapeclipper_hip.h"

namespace sc_mr {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int MAX_IMAGES = 65535;             // gridDim.y
constexpr int MAX_VIEWS = 65535;              // gridDim.z
constexpr int MAX_SIDE = 4096;
constexpr int WAVE_BLOCKS = 64;               // workgroups of the wave path per (image, view): 256 waves stride over the list
constexpr unsigned long long EMPTY = ~0ull;
constexpr float SNAP_LIMIT = 268435456.0f;    // 2^28
constexpr float F32_MAX = 3.402823466e+38f;

enum { DRAWN = 0, CULL_NEAR = 1, CULL_RANGE = 2, ZERO_AREA = 3 };

struct Layout {
    size_t keys, proj, large, cursor, total;
};

__host__ inline Layout layout(long long n_images, long long n_views, long long n_verts, long long n_faces, long long pixels) {
    Layout l;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += (bytes + 15) & ~(size_t)15; return here; };
    l.keys = take((size_t)(n_images * n_views * pixels) * 8);
    l.proj = take((size_t)(n_views * n_verts) * 16);
    l.large = take((size_t)(n_views * n_faces) * 4);
    l.cursor = take((size_t)(n_images * n_views) * 4);
    l.total = at;
    return l;
}

// the projected triangle, oriented counter-clockwise on the lattice (area > 0): vertex k at (x[k], y[k]), camera depth z[k];
// `swapped` when oriented vertices 1 and 2 are the face's vertices 2 and 1
struct Tri {
    long long x[3], y[3], area;
    float z[3];
    bool swapped;
};

// grid (ceil(n_verts / THREADS), n_views): thread = vertex g of the packed array, seen from view blockIdx.y of its image
__global__ void __launch_bounds__(THREADS) project_kernel(const float* __restrict__ verts, const long long* __restrict__ v_start,
                                                          const float* __restrict__ pose, const float* __restrict__ intr, int n_images,
                                                          long long n_verts, int n_views, float near, int4* __restrict__ proj) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= n_verts) return;
    const int view = blockIdx.y;
    int lo = 0, hi = n_images - 1;                    // the image of vertex g: the last b with v_start[b] <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (v_start[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const float* P = pose + 12 * ((long long)lo * n_views + view);
    const float* K = intr + 9 * (long long)lo;
    const float x = verts[3 * g], y = verts[3 * g + 1], z = verts[3 * g + 2];
    const float xc = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    const float yc = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    const float zc = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
    const float sx = (K[0] * xc) / zc + K[2];
    const float sy = (K[4] * yc) / zc + K[5];
    const float fx = rintf(sx * 256.0f), fy = rintf(sy * 256.0f);
    int flag = DRAWN;
    if (zc < near) flag = CULL_NEAR;
    else if (!(fabsf(zc) <= F32_MAX) || !(fabsf(fx) < SNAP_LIMIT) || !(fabsf(fy) < SNAP_LIMIT)) flag = CULL_RANGE;   // NaN fails every test
    const int X = flag == DRAWN ? (int)fx : 0, Y = flag == DRAWN ? (int)fy : 0;
    proj[(long long)view * n_verts + g] = make_int4(X, Y, __float_as_int(zc), flag);
}

// face `face` of image b from view `view` -> its category; t is set when DRAWN
__device__ __forceinline__ int load_tri(const int32_t* __restrict__ faces, const long long* __restrict__ v_start,
                                        const int4* __restrict__ proj, int n_images, long long n_verts, int b, int view, long long fbase,
                                        long long face, Tri& t) {
    const int32_t* fv = faces + 3 * (fbase + face);
    const long long vlo = v_start[b], vhi = b + 1 < n_images ? v_start[b + 1] : n_verts;
    int4 p[3];
    bool near = false, range = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        long long vi = vlo + (long long)fv[k];
        vi = vi > vhi - 1 ? vhi - 1 : vi;
        vi = vi < vlo ? vlo : vi;                                      // into the image's range ...
        vi = vi < 0 ? 0 : (vi >= n_verts ? n_verts - 1 : vi);         // ... and never outside verts
        p[k] = proj[(long long)view * n_verts + vi];
        near |= p[k].w == CULL_NEAR;
        range |= p[k].w == CULL_RANGE;
    }
    if (near) return CULL_NEAR;
    if (range) return CULL_RANGE;
    const long long ax = p[0].x, ay = p[0].y, bx = p[1].x, by = p[1].y, cx = p[2].x, cy = p[2].y;
    const long long area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    if (area == 0) return ZERO_AREA;
    t.swapped = area < 0;
    const int i1 = t.swapped ? 2 : 1, i2 = t.swapped ? 1 : 2;
    t.x[0] = ax; t.y[0] = ay; t.z[0] = __int_as_float(p[0].z);
    t.x[1] = p[i1].x; t.y[1] = p[i1].y; t.z[1] = __int_as_float(p[i1].z);
    t.x[2] = p[i2].x; t.y[2] = p[i2].y; t.z[2] = __int_as_float(p[i2].z);
    t.area = t.swapped ? -area : area;
    return DRAWN;
}

__device__ __forceinline__ long long lmin(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long lmax(long long a, long long b) { return a > b ? a : b; }

// the pixel columns [i0, i1] and rows [j0, j1] whose centres lie inside the triangle's bounding box, clamped to the image
__device__ __forceinline__ void pixel_box(const Tri& t, int H, int W, int& i0, int& i1, int& j0, int& j1) {
    const long long xmin = lmin(t.x[0], lmin(t.x[1], t.x[2])), xmax = lmax(t.x[0], lmax(t.x[1], t.x[2]));
    const long long ymin = lmin(t.y[0], lmin(t.y[1], t.y[2])), ymax = lmax(t.y[0], lmax(t.y[1], t.y[2]));
    const long long a = (xmin + 127) >> 8, b = (xmax - 128) >> 8;     // ceil((xmin - 128) / 256), floor((xmax - 128) / 256)
    const long long c = (ymin + 127) >> 8, d = (ymax - 128) >> 8;
    i0 = (int)lmax(a, 0); i1 = (int)lmin(b, (long long)W - 1);
    j0 = (int)lmax(c, 0); j1 = (int)lmin(d, (long long)H - 1);
}

// edge p -> q of the oriented triangle at the centre (Px, Py): inside, or on the edge and the edge is a top or a left one
__device__ __forceinline__ bool edge(long long px, long long py, long long qx, long long qy, long long Px, long long Py, long long& E) {
    const long long dx = qx - px, dy = qy - py;
    E = dx * (Py - py) - dy * (Px - px);
    return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

// pixel (i, j) against the triangle: covered?  depth and the barycentrics in the ORIENTED order when it is
__device__ __forceinline__ bool shade(const Tri& t, int i, int j, float& depth, float bary[3]) {
    const long long Px = 256LL * i + 128, Py = 256LL * j + 128;
    long long E0, E1, E2;                                               // E_k: the edge opposite oriented vertex k
    const bool in2 = edge(t.x[0], t.y[0], t.x[1], t.y[1], Px, Py, E2);
    const bool in0 = edge(t.x[1], t.y[1], t.x[2], t.y[2], Px, Py, E0);
    const bool in1 = edge(t.x[2], t.y[2], t.x[0], t.y[0], Px, Py, E1);
    if (!(in0 && in1 && in2)) return false;
    const float fa = (float)t.area;
    const float b0 = (float)E0 / fa, b1 = (float)E1 / fa, b2 = (float)E2 / fa;
    const float q0 = b0 / t.z[0], q1 = b1 / t.z[1], q2 = b2 / t.z[2];
    const float s = (q0 + q1) + q2;
    depth = 1.0f / s;
    bary[0] = q0 / s; bary[1] = q1 / s; bary[2] = q2 / s;
    return true;
}

__device__ __forceinline__ void publish(unsigned long long* __restrict__ keys, long long pixel, float depth, long long face) {
    atomicMin(&keys[pixel], ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned int)face);
}

// grid (ceil(n_faces / THREADS), n_images, n_views): thread = face f of image blockIdx.y from view blockIdx.z
__global__ void __launch_bounds__(THREADS) faces_kernel(const int32_t* __restrict__ faces, const long long* __restrict__ v_start,
                                                        const long long* __restrict__ f_start, const long long* __restrict__ f_count,
                                                        const int4* __restrict__ proj, int n_images, long long n_verts, long long n_faces,
                                                        int n_views, int H, int W, long long large_pixels,
                                                        unsigned long long* __restrict__ keys, int32_t* __restrict__ large,
                                                        int32_t* __restrict__ cursor, int32_t* __restrict__ stats) {
    const int b = blockIdx.y, view = blockIdx.z;
    const long long F = f_count[b], fbase = f_start[b];
    if ((long long)blockIdx.x * THREADS >= F) return;                   // the whole workgroup
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    const bool live = f < F && fbase >= 0 && fbase + f < n_faces;
    const int lane = threadIdx.x & (WAVE - 1);
    const long long bv = (long long)b * n_views + view;
    Tri t;
    const int cat = live ? load_tri(faces, v_start, proj, n_images, n_verts, b, view, fbase, f, t) : -1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {                                       // one integer add per wave and category
        const unsigned long long m = __ballot(cat == c);
        if (lane == 0 && m) atomicAdd(&stats[4 * bv + c], (int)__popcll(m));
    }
    int i0 = 0, i1 = -1, j0 = 0, j1 = -1;
    if (cat == DRAWN) pixel_box(t, H, W, i0, i1, j0, j1);
    const long long bw = i1 - i0 + 1, bh = j1 - j0 + 1;
    const long long n = (bw > 0 && bh > 0) ? bw * bh : 0;
    const bool listed = n > 0 && n > large_pixels;
    const unsigned long long m = __ballot(listed);
    if (m) {                                                            // the wave's listed faces take consecutive slots
        const int leader = __ffsll((long long)m) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&cursor[bv], (int)__popcll(m));
        base = __shfl(base, leader);
        if (listed) large[(long long)view * n_faces + fbase + base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)f;
    }
    if (n == 0 || listed) return;
    const long long pix0 = bv * H * W;
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) {
            float depth, bary[3];
            if (shade(t, i, j, depth, bary)) publish(keys, pix0 + (long long)j * W + i, depth, f);
        }
}

// grid (WAVE_BLOCKS, n_images, n_views): the waves of (image, view) stride over its list, a wave's lanes over a face's box
__global__ void __launch_bounds__(THREADS) wave_kernel(const int32_t* __restrict__ faces, const long long* __restrict__ v_start,
                                                       const long long* __restrict__ f_start, const long long* __restrict__ f_count,
                                                       const int4* __restrict__ proj, int n_images, long long n_verts, long long n_faces,
                                                       int n_views, int H, int W, unsigned long long* __restrict__ keys,
                                                       const int32_t* __restrict__ large, const int32_t* __restrict__ cursor) {
    const int b = blockIdx.y, view = blockIdx.z;
    const long long bv = (long long)b * n_views + view;
    const long long F = f_count[b], fbase = f_start[b];
    long long count = cursor[bv];
    count = count > F ? F : count;
    const int lane = threadIdx.x & (WAVE - 1);
    const long long pix0 = bv * H * W;
    for (long long e = (long long)blockIdx.x * (THREADS / WAVE) + (threadIdx.x >> 6); e < count; e += WAVE_BLOCKS * (THREADS / WAVE)) {
        const long long f = large[(long long)view * n_faces + fbase + e];
        if (f < 0 || f >= F || fbase < 0 || fbase + f >= n_faces) continue;
        Tri t;
        if (load_tri(faces, v_start, proj, n_images, n_verts, b, view, fbase, f, t) != DRAWN) continue;
        int i0, i1, j0, j1;
        pixel_box(t, H, W, i0, i1, j0, j1);
        const long long bw = i1 - i0 + 1, bh = j1 - j0 + 1;
        if (bw <= 0 || bh <= 0) continue;
        for (long long p = lane; p < bw * bh; p += WAVE) {
            const int j = j0 + (int)(p / bw), i = i0 + (int)(p - (p / bw) * bw);
            float depth, bary[3];
            if (shade(t, i, j, depth, bary)) publish(keys, pix0 + (long long)j * W + i, depth, f);
        }
    }
}

// grid (ceil(H W / THREADS), n_images, n_views): thread = pixel; the winner's depth and barycentrics are computed again from its face
__global__ void __launch_bounds__(THREADS) resolve_kernel(const int32_t* __restrict__ faces, const long long* __restrict__ v_start,
                                                          const long long* __restrict__ f_start, const long long* __restrict__ f_count,
                                                          const int4* __restrict__ proj, int n_images, long long n_verts, long long n_faces,
                                                          int n_views, int H, int W, const unsigned long long* __restrict__ keys,
                                                          int32_t* __restrict__ face_out, float* __restrict__ depth_out,
                                                          float* __restrict__ bary_out) {
    const int pixel = blockIdx.x * THREADS + threadIdx.x;
    if (pixel >= H * W) return;
    const int b = blockIdx.y, view = blockIdx.z;
    const long long at = ((long long)b * n_views + view) * H * W + pixel;
    const unsigned long long key = keys[at];
    int32_t face = -1;
    float depth = 0.0f, out[3] = {0.0f, 0.0f, 0.0f};
    const long long f = (long long)(key & 0xffffffffull), fbase = f_start[b];
    if (key != EMPTY && f < f_count[b] && fbase >= 0 && fbase + f < n_faces) {
        Tri t;
        float bary[3];
        const int j = pixel / W, i = pixel - j * W;
        if (load_tri(faces, v_start, proj, n_images, n_verts, b, view, fbase, f, t) == DRAWN && shade(t, i, j, depth, bary)) {
            face = (int32_t)f;
            out[0] = bary[0];
            out[1] = t.swapped ? bary[2] : bary[1];
            out[2] = t.swapped ? bary[1] : bary[2];
        } else {
            depth = 0.0f;
        }
    }
    face_out[at] = face;
    depth_out[at] = depth;
    bary_out[3 * at] = out[0]; bary_out[3 * at + 1] = out[1]; bary_out[3 * at + 2] = out[2];
}

__host__ inline bool sizes_ok(int n_images, long long n_verts, long long n_faces, int n_views, int height, int width) {
    return n_images <= MAX_IMAGES && n_views >= 1 && n_views <= MAX_VIEWS && height >= 1 && height <= MAX_SIDE && width >= 1 &&
           width <= MAX_SIDE && n_verts <= (1LL << 31) && n_faces <= (1LL << 31) &&
           (n_images <= 0 || (long long)n_images * n_views <= (1LL << 40) / ((long long)height * width));
}

}  // namespace sc_mr

extern "C" long long sc_mesh_raster_scratch_bytes(int n_images, int n_views, long long n_verts, long long n_faces, int height, int width) {
    using namespace sc_mr;
    if (!sizes_ok(n_images, n_verts, n_faces, n_views, height, width)) return -1;
    if (n_images <= 0 || n_verts <= 0 || n_faces <= 0) return 0;
    return (long long)layout(n_images, n_views, n_verts, n_faces, (long long)height * width).total;
}

extern "C" int sc_mesh_raster(const float* verts, const int32_t* faces, const long long* v_start, const long long* f_start,
                              const long long* f_count, const float* pose, const float* intr, int n_images, long long n_verts,
                              long long n_faces, int n_views, int height, int width, float near, long long large_pixels, int32_t* face,
                              float* depth, float* bary, int32_t* stats, void* scratch, void* stream) {
    using namespace sc_mr;
    if (!sizes_ok(n_images, n_verts, n_faces, n_views, height, width) || !(near > 0.0f)) return (int)hipErrorInvalidValue;
    if (n_images <= 0 || n_verts <= 0 || n_faces <= 0) return 0;
    if (!verts || !faces || !v_start || !f_start || !f_count || !pose || !intr || !face || !depth || !bary || !stats || !scratch ||
        ((uintptr_t)scratch & 15))
        return (int)hipErrorInvalidValue;
    const hipStream_t s = (hipStream_t)stream;
    const long long pixels = (long long)height * width;
    const Layout l = layout(n_images, n_views, n_verts, n_faces, pixels);
    char* ws = (char*)scratch;
    unsigned long long* keys = (unsigned long long*)(ws + l.keys);
    int4* proj = (int4*)(ws + l.proj);
    int32_t* large = (int32_t*)(ws + l.large);
    int32_t* cursor = (int32_t*)(ws + l.cursor);
    hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)n_images * n_views * pixels * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(cursor, 0, (size_t)n_images * n_views * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(stats, 0, (size_t)n_images * n_views * 16, s);
    if (e != hipSuccess) return (int)e;
    const dim3 block(THREADS);
    hipLaunchKernelGGL(project_kernel, dim3((unsigned int)((n_verts + THREADS - 1) / THREADS), (unsigned int)n_views), block, 0, s, verts,
                       v_start, pose, intr, n_images, n_verts, n_views, near, proj);
    hipLaunchKernelGGL(faces_kernel, dim3((unsigned int)((n_faces + THREADS - 1) / THREADS), (unsigned int)n_images, (unsigned int)n_views),
                       block, 0, s, faces, v_start, f_start, f_count, proj, n_images, n_verts, n_faces, n_views, height, width,
                       large_pixels, keys, large, cursor, stats);
    hipLaunchKernelGGL(wave_kernel, dim3(WAVE_BLOCKS, (unsigned int)n_images, (unsigned int)n_views), block, 0, s, faces, v_start, f_start,
                       f_count, proj, n_images, n_verts, n_faces, n_views, height, width, keys, large, cursor);
    hipLaunchKernelGGL(resolve_kernel, dim3((unsigned int)((pixels + THREADS - 1) / THREADS), (unsigned int)n_images, (unsigned int)n_views),
                       block, 0, s, faces, v_start, f_start, f_count, proj, n_images, n_verts, n_faces, n_views, height, width, keys, face,
                       depth, bary);
    return (int)hipGetLastError();
}
