/* shapeclipper_hip.h -- C ABI of libshapeclipper_hip.so (hand-written gfx950 / MI355X kernels).
 *
 * Drop-in boundary for the ShapeClipper hot path.  Plain pointers and sizes only: every pointer is
 * a DEVICE pointer into memory the caller owns (nothing is allocated or freed inside, there is no
 * global state, calls are re-entrant per device), `stream` is a hipStream_t (pass torch's current
 * stream), and the caller has already made the right device current.  Return value: 0 on success,
 * otherwise the hipError_t of the failed launch (the Python side raises).
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   sc_chamfer3d_forward   <- chamfer_3D.forward  (external/chamfer3D/chamfer_cuda.cpp:17-19,31;
 *                                                  kernel chamfer3D.cu:12-154)
 *   sc_chamfer3d_backward  <- chamfer_3D.backward (chamfer_cuda.cpp:22-27,32; chamfer3D.cu:155-195)
 *   sc_sdf_forward         <- SDFNetwork.get_conditional_output (model/implicit.py:163-189) and
 *                             compute_level_grid's inner call (utils/eval_3D.py:21-38)
 *   sc_sdf_backward        <- autograd of the above incl. the create_graph=True double backward
 *   sc_render_*            <- Renderer.forward (model/renderer.py:57-185) and its autograd
 *   sc_loss_*              <- Loss.MSE_loss / mask_loss / normal_loss (model/loss.py:19-97)
 */
#ifndef SHAPECLIPPER_HIP_H
#define SHAPECLIPPER_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Chamfer3D.  xyz1 [b,n,3], xyz2 [b,m,3] fp32 contiguous.  dist1 [b,n], dist2 [b,m]: SQUARED
 * nearest-neighbour distance d = fma(dy,dy,dx*dx) + dz*dz (the reference extension's arithmetic on this GPU: oracle/chamfer_ref.c); idx1 [b,n], idx2 [b,m] int32: index
 * of the nearest neighbour, lowest index among exact ties (chamfer3D.cu:36,126).  Outputs are
 * fully overwritten (if n==0 or m==0 they are left untouched, as the reference does).
 * Launches on `stream` (the reference used the legacy default stream).                          */
int sc_chamfer3d_forward(const float* xyz1, const float* xyz2, float* dist1, float* dist2,
                         int32_t* idx1, int32_t* idx2, int b, int n, int m, void* stream);

/* Same results (bit for bit): the targets are split over `nsplit` workgroup slices and merged with 64-bit atomicMin on
 * (distance bits, index) keys; nsplit <= 0: chosen per direction so that the launch is a whole number of full rounds of the
 * chip (5 workgroups per CU at a time).  workspace: (b*n + b*m) * 8 bytes of device scratch.   */
int sc_chamfer3d_forward_split(const float* xyz1, const float* xyz2, float* dist1, float* dist2,
                               int32_t* idx1, int32_t* idx2, int b, int n, int m, int nsplit,
                               void* workspace, void* stream);

/* Same results (bit for bit) from an exact accelerated search (csrc/chamfer_grid.hip): each cloud is binned into a uniform
 * grid and every query walks rings of cells around its own, evaluating candidates with the same expression and accepting on
 * d < best || (d == best && index < best_index); the walk stops only when no unseen target can tie or beat the best (rounding
 * of the binning and of d included).  Queries that do not terminate within a few rings (far outside the other cloud, one huge
 * cell, non-finite coordinates) are answered by the brute-force scan, so the worst case is about sc_chamfer3d_forward's cost.
 * Surface-like targets (>= 8 per occupied cell: the evaluation's clouds) are walked one wave per 64 queries of a 2 x 2 x 2 tile of cells.
 * workspace: sc_chamfer3d_grid_workspace_bytes(b, n, m) bytes of device scratch (contents irrelevant on entry).       */
long long sc_chamfer3d_grid_workspace_bytes(int b, int n, int m);
int sc_chamfer3d_forward_grid(const float* xyz1, const float* xyz2, float* dist1, float* dist2,
                              int32_t* idx1, int32_t* idx2, int b, int n, int m, void* workspace, void* stream);

/* gradxyz1 [b,n,3], gradxyz2 [b,m,3] must be ZERO-FILLED by the caller (atomicAdd accumulation,
 * chamfer3D.cu:166-171,177-178).                                                                */
int sc_chamfer3d_backward(const float* xyz1, const float* xyz2, float* gradxyz1, float* gradxyz2,
                          const float* graddist1, const float* graddist2, const int32_t* idx1,
                          const int32_t* idx2, int b, int n, int m, void* stream);

/* The same gradient without float atomics, bitwise reproducible (csrc/chamfer_bwd.hip).  gradxyz1 / gradxyz2 are OVERWRITTEN:
 * unlike sc_chamfer3d_backward there is no zero-fill contract, whatever they held on entry is gone.  Either may be NULL: that
 * cloud's gradient is not formed and its passes are skipped.  Indices must satisfy 0 <= idx1 < m, 0 <= idx2 < n (what the
 * forward entry points write).
 * The term of source j of cloud 1 with k = idx1[b,j] is t = (2 * graddist1[b,j]) * (xyz1[b,j] - xyz2[b,k]), per component, every
 * operation rounded to fp32 on its own (no fused multiply-add); direction 2 is the mirror image with idx2 / graddist2.
 * Summation order, a function of the inputs only (not of b, the chip, the stream or sc_set_reserved_cus):
 *   row gradxyz1[b,j] = t(j) + S, where S sums the terms -t(i) of the sources i of cloud 2 with idx2[b,i] == j (gradxyz2 alike);
 *   the sources of a row are taken in ASCENDING source index and cut into chunks of C = sc_chamfer3d_backward_ordered_chunk()
 *   consecutive list entries (the last one shorter); a chunk's partial sum is P = ((+0 + u0) + u1) + ... over its entries in
 *   order, and S = ((+0 + P0) + P1) + ... over the chunks in order (S = +0 for a row nobody points at).
 * b <= 0 returns 0 and writes nothing; n == 0 or m == 0 writes zeros to the non-empty gradient that was given (an empty opposite
 * cloud gives no terms).  workspace: sc_chamfer3d_backward_ordered_workspace_bytes(b, n, m) bytes of device scratch, contents
 * irrelevant on entry, the same size whichever gradients are asked for; nothing is allocated inside.  Launches on `stream`.  */
long long sc_chamfer3d_backward_ordered_workspace_bytes(int b, int n, int m);
int sc_chamfer3d_backward_ordered_chunk(void);
int sc_chamfer3d_backward_ordered(const float* xyz1, const float* xyz2, float* gradxyz1, float* gradxyz2,
                                  const float* graddist1, const float* graddist2, const int32_t* idx1,
                                  const int32_t* idx2, int b, int n, int m, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Conditional SDF MLP, shipped architecture only (options/pix3d/config.yaml: 5 hidden x 64,
 * softplus(100), skips at layers 1,2, pos_enc 6, force_symmetry).
 *
 * w_pack  : kernel-ready weight image, SC_SDF_PACK_FLOATS floats (layout: mlp_tile.hpp SdfPack;
 *           produced by shapeclipper_amd.packing.pack_sdf -- PE columns in slot order, skip
 *           scale 1/sqrt(2) applied, latent columns removed).
 * cbias   : [n_images][5][64] per-image biases c_l = b_l + W_l[:, latent] z (scaled for skips).
 * points  : [n_points][3], image-major; image(i) = min(i / n_per_image, n_images-1).
 * Outputs (any may be NULL):  sdf [n_points];  grad [n_points][3] = d sdf / d point (its presence
 * selects the gradient kernel);  feat / stash_a / stash_p: tile-blocked 64-channel tensors
 * (TBL64: [ceil(n/16)][16][16][4] floats), stash_a holds 5 and stash_p 4 such tensors back to back
 * (since round 5 the ACTIVATIONS h_0..h_4 = softplus(a_l) -- a_l before -- and the adjoints p_0..p_3, kept for sc_sdf_backward[_fused]: with
 * u = exp(-100 h) the reverse passes get sp'(a) = 1 - u and sp''(a) = 100 (1 - u) u from ONE transcendental and sp(a) = h from none; the buffer
 * is opaque to callers: whatever sc_sdf_forward wrote is what the backward entry points of the SAME library build read).
 * scratch: required when grad != NULL and stash_a == NULL: 256*8*5*1024 floats of per-wave scratch.  */
#define SC_SDF_PACK_FLOATS (64*48 + 2*64*112 + 2*64*64 + 65*64 + 65)
#define SC_RGB_PACK_FLOATS (64*112 + 2*64*64 + 3*64 + 4)
#define SC_TILE_POINTS 16
int sc_sdf_forward(const float* points, const float* w_pack, const float* cbias, int n_points,
                   int n_per_image, int n_images, int symmetric, float* sdf, float* grad,
                   float* feat, float* stash_a, float* stash_p, float* scratch, void* stream);

/* Reverse pass of sc_sdf_forward incl. the second-order terms of d/dtheta[d sdf/dx] (what autograd's
 * double backward does for model/implicit.py:180-186 + model/renderer.py:101-107).
 * stash_a / stash_p: as written by sc_sdf_forward.  g_sdf [n], g_grad [n][3], g_feat (TBL64): upstream
 * gradients, any may be NULL (= zero).  Outputs: g_points [n][3] (may be NULL); ga (5 x TBL64), gp (4 x
 * TBL64, only written when g_grad != NULL), r0 (TBL64): operands of the weight-gradient GEMMs (sc_wgrad). */
int sc_sdf_backward(const float* points, const float* w_pack, int n_points, int symmetric,
                    const float* stash_a, const float* stash_p, const float* g_sdf, const float* g_grad,
                    const float* g_feat, float* g_points, float* ga, float* gp, float* r0, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RGB MLP + Laplace density + alpha compositing, one wavefront per ray of 64 samples
 * (RGBNetwork.forward model/implicit.py:220-239, LaplaceDensity :65-83, Renderer.volume_rendering
 * model/renderer.py:187-209 and the per-ray reductions :117-152).
 * points [n_rays*64][3], z_vals [n_rays][64], depth_fac [n_rays], sdf [P], grad [P][3] (= d sdf/dx),
 * feat TBL64 (from sc_sdf_forward), v_pack (SC_RGB_PACK_FLOATS, packing.pack_rgb), dbias
 * [n_images][3][64], beta_param: the raw scalar parameter renderer.density.beta in device memory.
 * Outputs: rgb [n_rays][3], mask/mask_hard/depth [n_rays], normal [n_rays][3]; optional weights/alpha
 * [n_rays][64] and rgb_flat [P][3] (rgb_flat is required by the backward).                          */
int sc_rgb_composite_forward(const float* points, const float* z_vals, const float* depth_fac,
                             const float* sdf, const float* grad, const float* feat,
                             const float* v_pack, const float* dbias, const float* beta_param,
                             int n_rays, int rays_per_image, int n_images, int symmetric,
                             float beta_min, float bgcolor, float normal_pow,
                             float* rgb, float* mask, float* mask_hard, float* depth, float* normal,
                             float* weights, float* alpha, float* rgb_flat, void* stream);
/* The same, and the post-ReLU activations r0, r1, r2 of the three hidden layers of RGBNetwork (model/implicit.py:233-237) are parked in
 * rr (3 x TBL64 = 3 x n_rays * 4 * 1024 floats, layer-major; NULL = not parked) for sc_rgb_composite_backward_fused_stash.        */
int sc_rgb_composite_forward_stash(const float* points, const float* z_vals, const float* depth_fac,
                                   const float* sdf, const float* grad, const float* feat,
                                   const float* v_pack, const float* dbias, const float* beta_param,
                                   int n_rays, int rays_per_image, int n_images, int symmetric,
                                   float beta_min, float bgcolor, float normal_pow,
                                   float* rgb, float* mask, float* mask_hard, float* depth, float* normal,
                                   float* weights, float* alpha, float* rgb_flat, float* rr, void* stream);
/* round 6: sc_rgb_composite_forward_stash with the RGB network in the exact three-piece bf16 split arithmetic, weights pre-split in LDS
 * (csrc/mlp_presplit.hpp; six piece products per fp32 product on the bf16 matrix pipe, fp32 accumulation -- error against float64 that of
 * the fp32 chain).  Same operands and outputs; mask / mask_hard / depth / normal do not depend on the RGB network and are bit-identical
 * to the fp32-MFMA form's, the colours differ by fp32 rounding.                                                                         */
int sc_rgb_composite_forward_split(const float* points, const float* z_vals, const float* depth_fac,
                                   const float* sdf, const float* grad, const float* feat,
                                   const float* v_pack, const float* dbias, const float* beta_param,
                                   int n_rays, int rays_per_image, int n_images, int symmetric,
                                   float beta_min, float bgcolor, float normal_pow,
                                   float* rgb, float* mask, float* mask_hard, float* depth, float* normal,
                                   float* weights, float* alpha, float* rgb_flat, float* rr, void* stream);

/* Sample counts other than 64.  The _ns entry points below take n_samples = S, the samples per ray, right after n_rays; every
 * "64" in the shapes above becomes S (points [n_rays*S][3], z_vals [n_rays][S], TBL64 tensors n_rays * (S / 16) * 1024 floats).
 * S must satisfy SC_N_SAMPLES_SUPPORTED (a multiple of 32 in [32, 256]); any other S returns hipErrorInvalidValue before anything
 * is launched.  S = 64 runs exactly the kernels of the symbols without _ns, which are these entry points with S = 64.             */
#define SC_N_SAMPLES_SUPPORTED(n) ((n) >= 32 && (n) <= 256 && (n) % 32 == 0)
int sc_rgb_composite_forward_ns(const float* points, const float* z_vals, const float* depth_fac,
                                const float* sdf, const float* grad, const float* feat,
                                const float* v_pack, const float* dbias, const float* beta_param,
                                int n_rays, int n_samples, int rays_per_image, int n_images, int symmetric,
                                float beta_min, float bgcolor, float normal_pow,
                                float* rgb, float* mask, float* mask_hard, float* depth, float* normal,
                                float* weights, float* alpha, float* rgb_flat, void* stream);
int sc_rgb_composite_forward_stash_ns(const float* points, const float* z_vals, const float* depth_fac,
                                      const float* sdf, const float* grad, const float* feat,
                                      const float* v_pack, const float* dbias, const float* beta_param,
                                      int n_rays, int n_samples, int rays_per_image, int n_images, int symmetric,
                                      float beta_min, float bgcolor, float normal_pow,
                                      float* rgb, float* mask, float* mask_hard, float* depth, float* normal,
                                      float* weights, float* alpha, float* rgb_flat, float* rr, void* stream);
int sc_rgb_composite_forward_split_ns(const float* points, const float* z_vals, const float* depth_fac,
                                      const float* sdf, const float* grad, const float* feat,
                                      const float* v_pack, const float* dbias, const float* beta_param,
                                      int n_rays, int n_samples, int rays_per_image, int n_images, int symmetric,
                                      float beta_min, float bgcolor, float normal_pow,
                                      float* rgb, float* mask, float* mask_hard, float* depth, float* normal,
                                      float* weights, float* alpha, float* rgb_flat, float* rr, void* stream);

/* Reverse pass.  G_* are the upstream per-ray gradients (NULL = zero).  g_beta: SC_RGB_BWD_BETA_PARTS floats, fully
 * written: one partial of d/d(raw beta parameter) per wave of the grid; the gradient is their sum in index order
 * (sc_partial_reduce(g_beta, SC_RGB_BWD_BETA_PARTS, 1, 1, out)) -- a fixed summation order, no float atomics.
 * gy (3 x TBL64), rr (3 x TBL64), gy3 [P][3]: operands for the RGB weight gradients.                          */
#define SC_RGB_BWD_BETA_PARTS 2048
int sc_rgb_composite_backward(
    const float* points, const float* z_vals, const float* depth_fac, const float* sdf, const float* grad,
    const float* feat, const float* v_pack, const float* dbias, const float* beta_param, const float* rgb_flat,
    int n_rays, int rays_per_image, int n_images, int symmetric, float beta_min, float bgcolor, float normal_pow,
    const float* G_rgb, const float* G_mask, const float* G_depth, const float* G_normal,
    float* g_sdf, float* g_grad, float* g_feat, float* g_points, float* g_z, float* g_depth_fac, float* g_beta,
    float* gy, float* rr, float* gy3, void* stream);
/* The same with the gradient of the 3-row output layer folded in: v3_part [SC_RGB_BWD_BETA_PARTS][196] (fully written) holds, per wave of
 * the grid, the sums over its points of gy3_j * r2[ch] (dV3 [3][64]), of gy3_j (db3 [3]) and a zero; the gradient is their sum in index
 * order (sc_partial_reduce(v3_part, SC_RGB_BWD_BETA_PARTS, 196, 196, out)).  rr[2] and gy3 are then NOT written (may be NULL past rr[1]).
 * v3_part == NULL: exactly sc_rgb_composite_backward.                                                                                  */
int sc_rgb_composite_backward_v3(
    const float* points, const float* z_vals, const float* depth_fac, const float* sdf, const float* grad,
    const float* feat, const float* v_pack, const float* dbias, const float* beta_param, const float* rgb_flat,
    int n_rays, int rays_per_image, int n_images, int symmetric, float beta_min, float bgcolor, float normal_pow,
    const float* G_rgb, const float* G_mask, const float* G_depth, const float* G_normal,
    float* g_sdf, float* g_grad, float* g_feat, float* g_points, float* g_z, float* g_depth_fac, float* g_beta,
    float* gy, float* rr, float* gy3, float* v3_part, void* stream);

/* The same reverse pass with the weight gradients of V0, V1, V2 and the per-image bias gradients formed INSIDE the kernel (round 5: four
 * weight-gradient waves beside the four chain waves, operands handed over through LDS -- the scheme of sc_sdf_backward_fused) instead of
 * the gy / rr hand-off tensors and three sc_wgrad launches.  partial: [sc_rgb_composite_backward_fused_parts(n_rays)]
 * [sc_rgb_composite_backward_fused_partial_floats(n_images)] floats, one image per workgroup = d/d(V0 | V1 | V2) (RgbPack order, 15,360
 * floats) then [n_images][3][64] bias gradients, fully written; sum them in index order (sc_partial_reduce).  v3_part as above.
 * n_images <= 256.                                                                                                             */
int sc_rgb_composite_backward_fused_parts(int n_rays);
int sc_rgb_composite_backward_fused_partial_floats(int n_images);
int sc_rgb_composite_backward_fused(
    const float* points, const float* z_vals, const float* depth_fac, const float* sdf, const float* grad,
    const float* feat, const float* v_pack, const float* dbias, const float* beta_param, const float* rgb_flat,
    int n_rays, int rays_per_image, int n_images, int symmetric, float beta_min, float bgcolor, float normal_pow,
    const float* G_rgb, const float* G_mask, const float* G_depth, const float* G_normal,
    float* g_sdf, float* g_grad, float* g_feat, float* g_points, float* g_z, float* g_depth_fac, float* g_beta,
    float* partial, float* v3_part, void* stream);
/* sc_rgb_composite_backward_fused reading the hidden activations the forward pass parked (rr of sc_rgb_composite_forward_stash) instead
 * of recomputing the forward chain (a third of the kernel's time); same outputs, same summation orders.                            */
int sc_rgb_composite_backward_fused_stash(
    const float* points, const float* z_vals, const float* depth_fac, const float* sdf, const float* grad,
    const float* feat, const float* v_pack, const float* dbias, const float* beta_param, const float* rgb_flat,
    int n_rays, int rays_per_image, int n_images, int symmetric, float beta_min, float bgcolor, float normal_pow,
    const float* G_rgb, const float* G_mask, const float* G_depth, const float* G_normal,
    float* g_sdf, float* g_grad, float* g_feat, float* g_points, float* g_z, float* g_depth_fac, float* g_beta,
    float* partial, float* v3_part, const float* rr, void* stream);
/* round 6: the same reverse pass with its three transposed products (V2^T, V1^T, V0f^T) and the encoding's Jacobian in the exact bf16x3
 * split arithmetic from pre-split fragments (csrc/mlp_presplit.hpp); same operands and outputs, gradients equal up to fp32 rounding.     */
int sc_rgb_composite_backward_fused_split(
    const float* points, const float* z_vals, const float* depth_fac, const float* sdf, const float* grad,
    const float* feat, const float* v_pack, const float* dbias, const float* beta_param, const float* rgb_flat,
    int n_rays, int rays_per_image, int n_images, int symmetric, float beta_min, float bgcolor, float normal_pow,
    const float* G_rgb, const float* G_mask, const float* G_depth, const float* G_normal,
    float* g_sdf, float* g_grad, float* g_feat, float* g_points, float* g_z, float* g_depth_fac, float* g_beta,
    float* partial, float* v3_part, const float* rr, void* stream);

/* The four reverse forms at S samples per ray (see SC_N_SAMPLES_SUPPORTED above); g_z is [n_rays][S].  Same summation orders: the
 * per-wave g_beta / v3_part partials and the per-workgroup partial images are what the S = 64 forms write.                      */
int sc_rgb_composite_backward_v3_ns(
    const float* points, const float* z_vals, const float* depth_fac, const float* sdf, const float* grad,
    const float* feat, const float* v_pack, const float* dbias, const float* beta_param, const float* rgb_flat,
    int n_rays, int n_samples, int rays_per_image, int n_images, int symmetric, float beta_min, float bgcolor, float normal_pow,
    const float* G_rgb, const float* G_mask, const float* G_depth, const float* G_normal,
    float* g_sdf, float* g_grad, float* g_feat, float* g_points, float* g_z, float* g_depth_fac, float* g_beta,
    float* gy, float* rr, float* gy3, float* v3_part, void* stream);
int sc_rgb_composite_backward_fused_ns(
    const float* points, const float* z_vals, const float* depth_fac, const float* sdf, const float* grad,
    const float* feat, const float* v_pack, const float* dbias, const float* beta_param, const float* rgb_flat,
    int n_rays, int n_samples, int rays_per_image, int n_images, int symmetric, float beta_min, float bgcolor, float normal_pow,
    const float* G_rgb, const float* G_mask, const float* G_depth, const float* G_normal,
    float* g_sdf, float* g_grad, float* g_feat, float* g_points, float* g_z, float* g_depth_fac, float* g_beta,
    float* partial, float* v3_part, void* stream);
int sc_rgb_composite_backward_fused_stash_ns(
    const float* points, const float* z_vals, const float* depth_fac, const float* sdf, const float* grad,
    const float* feat, const float* v_pack, const float* dbias, const float* beta_param, const float* rgb_flat,
    int n_rays, int n_samples, int rays_per_image, int n_images, int symmetric, float beta_min, float bgcolor, float normal_pow,
    const float* G_rgb, const float* G_mask, const float* G_depth, const float* G_normal,
    float* g_sdf, float* g_grad, float* g_feat, float* g_points, float* g_z, float* g_depth_fac, float* g_beta,
    float* partial, float* v3_part, const float* rr, void* stream);
int sc_rgb_composite_backward_fused_split_ns(
    const float* points, const float* z_vals, const float* depth_fac, const float* sdf, const float* grad,
    const float* feat, const float* v_pack, const float* dbias, const float* beta_param, const float* rgb_flat,
    int n_rays, int n_samples, int rays_per_image, int n_images, int symmetric, float beta_min, float bgcolor, float normal_pow,
    const float* G_rgb, const float* G_mask, const float* G_depth, const float* G_normal,
    float* g_sdf, float* g_grad, float* g_feat, float* g_points, float* g_z, float* g_depth_fac, float* g_beta,
    float* partial, float* v3_part, const float* rr, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight-gradient GEMM  dW[64][nb0+nb1] = sum_points A(p) (x) [B0(p) | B1(p)]  over one or two terms.
 * Operand transform codes: 1 plain TBL64, 2 softplus(a), 3 p*softplus'(a), 4 w5row*softplus'(a),
 * 5 positional encoding of the point (48 columns), 6 g_grad-weighted PE Jacobian (48 columns).
 * Every one of the `nparts` workgroups writes its partial result at
 * partial[part*partial_stride + out_offset + row*out_ld + col]; sc_partial_reduce sums the parts.
 * rowsum (may be NULL): [nparts * 4][n_images][64], fully written: per WAVE of the grid and per image, the sum over
 * the wave's points of term 0's A operand (= the bias / per-image latent gradient of that layer) -- the operand is in
 * registers anyway; the caller adds the nparts * 4 partial images in index order (sc_partial_reduce): a fixed summation
 * order instead of float atomics.  Requires n_per_image % 16 == 0 (a 16-point tile never straddles two images).       */
int sc_wgrad(int nterms,
             const float* a0_0, const float* a1_0, int aop_0, const float* b0_0, int bop0_0, const float* b1_0, int bop1_0,
             const float* a0_1, const float* a1_1, int aop_1, const float* b0_1, int bop0_1, const float* b1_1, int bop1_1,
             const float* points, const float* g_grad, const float* w5row, int n_points, int symmetric,
             int nb0, int nb1, float* partial, int nparts, int partial_stride, int out_offset, int out_ld,
             float* rowsum, int n_per_image, int n_images, void* stream);
/* out[i] = sum_part partial[part*stride + i], i < n, in a fixed order (interleaved sequential sums combined by a fixed binary tree):
 * results do not depend on timing.  out is assigned (need not be zero-filled).                              */
int sc_partial_reduce(const float* partial, int nparts, int stride, int n, float* out, void* stream);

/* out_t[img][k][ch] += sum_{p in img} coef[p][k] * x_t[ch][p] for t < n_tensors (<= 8) TBL64 tensors in ONE
 * launch (coef NULL: K = 1, coefficient 1; else K = 3).  xs / outs are HOST arrays of device pointers; every
 * Two modes.  part != NULL (needs n_per_image % 16 == 0): fixed summation order -- every block writes a partial image into
 * `part` (sc_tbl_sum_blocks(n_points) * n_tensors * n_images * K * 64 floats of workspace) and a second launch adds them in
 * block order into outs[0], which must be ONE buffer holding all tensors back to back ([n_tensors][n_images][K][64], fully
 * written).  part == NULL: every outs[t] must be zero-filled, float atomicAdd (summation order depends on timing).
 * Used for bias / latent gradients and the 3-row output layer of the RGB net.                                   */
int sc_tbl_sum_blocks(int n_points);
int sc_tbl_sum(const float* const* xs, int n_tensors, const float* coef, int n_points, int n_per_image,
               int n_images, float* const* outs, float* part, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Loss reductions of one render in one launch (Loss.MSE_loss / mask_loss / normal_loss, model/loss.py:19-97
 * as called from Graph.compute_loss, model/graph.py:224-236, 252-264).
 * rgb, rgb_t, normal, normal_t [B][R][3]; mask, mask_t [B][R]; eik [B][E] or NULL.
 * normal mask = (mask_t > 0.5) & (mask > 0.5); keep_frac = 1 - reg.normal_tol (double: the cut is
 * int(n * keep_frac) as in loss.py:62).  out4: EIGHT floats, zero-filled by the caller: [0..3] receive
 * (render MSE, IoU + mask_mse*MSE, robust normal loss, eikonal MSE), [4] is the arrival counter of the fixed-order
 * reduction over the images (results do not depend on timing), [5..7] pad; g_* receive d loss_k / d prediction;
 * g_normal_t [B][R][3] (or NULL) receives d normal loss / d normal_t -- the target is
 * camera.transform_normal(input normal, predicted pose) (graph.py:85,260), so autograd carries it into the estimator.
 * ang_ws: B*R + 4*B floats of workspace.                                                           */
int sc_loss_fused_forward(const float* rgb, const float* rgb_t, const float* mask, const float* mask_t,
                          const float* normal, const float* normal_t, const float* eik, int B, int R, int E,
                          float normal_l1, float mask_mse, double keep_frac, float* out4, float* g_rgb,
                          float* g_mask, float* g_normal, float* g_eik, float* g_normal_t, float* ang_ws,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * CLIP ViT image tower forward (replaces clip_encoder.encode_image, CLIP_anno.py:166; third-party
 * openai/CLIP, parity unpinned).  image [B][C][H][W] fp32 (already CLIP-normalised) -> out [B][proj_dim]
 * fp32 (NOT L2-normalised).  Requirements: head dim 64, D % 64 == 0, mlp % 64 == 0; any token count
 * T = (H/patch)*(W/patch)+1 whose transposed V tile fits LDS (ViT-B/32: 50, ViT-L/14: 257).
 * w_bf16: bf16 matrices, row-major [out][in], in this order: patch [D][Kp], Kp = C*patch*patch rounded up to a
 *   multiple of 64 with zero columns; per layer
 *   qkv [3D][D] (q rows, k rows, v rows), out_proj [D][D], fc1 [mlp][D], fc2 [D][mlp]; then proj [proj_dim][D].
 * w_f32: fp32 vectors in this order: class_embedding [D], position_embedding [T][D], ln_pre gamma, beta;
 *   per layer ln_1 gamma, beta, qkv bias [3D], out_proj bias, ln_2 gamma, beta, fc1 bias [mlp], fc2 bias;
 *   then ln_post gamma, beta.
 * workspace: >= sc_clip_vit_workspace_bytes(...) bytes of device memory.  It begins with the patch matrix [B*(T-1)][Kp] (16 bit), the
 *   patch embeddings [B*(T-1)][D] fp32 and the residual stream x [B*T][D] fp32 (after the call: the last layer's output; layers == 0:
 *   ln_pre's), each rounded up to 256 bytes.
 * Token-count branches of the attention stage (one workgroup per image and head; Tp = T rounded up to 32):
 *   T <= 32 or T > 64   attention_kernel: V^T [64][Tp + 4] in LDS, two passes over the keys in chunks of 32, a masked last chunk
 *                       when T % 32 != 0; query blocks of 32 go round-robin over eight waves;
 *   32 < T <= 64        attention_small_kernel: both key chunks in registers, one pass;
 *   272 Tp + 512 <= 160 KiB (T <= 576)   K is staged in LDS beside V^T; above (T = 577: ViT-L/14 at 336 x 336) both passes read K
 *                       from global memory;
 *   K in LDS, more than 8 query blocks and (number of query blocks) % 8 == 1 (T = 257..288, 513..544)   the last query block is
 *                       split over the KEYS: the eight waves' partial (max, sum, O) are merged in wave order through LDS;
 *   128 (Tp + 4) > 160 KiB (T > 1248)   refused (hipErrorInvalidValue).
 * LayerNorm: D % 256 == 0 and D <= 1024 with stride % 4 == 0 keeps the row in registers; any other D re-reads the row.  Both take
 * the mean first and then the centred squares (fp32).                                                   */
long long sc_clip_vit_workspace_bytes(int B, int C, int H, int W, int patch, int D, int mlp);
int sc_clip_vit_forward(const float* image, int B, int C, int H, int W, int patch, int D, int mlp, int layers,
                        int heads, int proj_dim, const uint16_t* w_bf16, const float* w_f32, float ln_eps,
                        float* out, void* workspace, long long workspace_bytes, void* stream);
/* out[M][N] = A[M][K] (bf16) * Wt[N][K]^T (bf16) + bias (bias may be NULL); epi 0: fp32 store, 1: fp32 +=, 2: quick_gelu -> bf16,
 * 3: bf16.  M, N, K > 0, K % 64 == 0 and 0 <= epi <= 3, anything else is refused (hipErrorInvalidValue, nothing launched).
 * Kernel branches (one decision, gemm_plan in csrc/clip_vit.hip, which sc_gemm_plan reports; first match wins):
 *   t128 = ceil(N/128) ceil(M/128), t256 = (N/256) ceil(M/256), t192 = (N/192) ceil(M/256); `fits`: (M + 256) N 4, (M + 256) K 2 and
 *   N K 2 bytes each below 4 GiB (32-bit offsets of the buffer resource and the LDS-DMA)
 *   gemm8p      N % 256 == 0, M >= 2048, t256 >= 200 (SC_GEMM_G8_MIN), fits: gemm8p_kernel, 256 x 256 tiles walked by one workgroup per
 *               CU (grid = CUs rounded down to 8).  Its last M % 256 rows go to a `thin` tail when they are at most 64, N % 32 == 0,
 *               K % 256 == 0 and the ragged row tile would open another round of that grid;
 *   gemm8p_192  epi 0 / 1, N % 192 == 0, M >= 2048, 180 <= t192 <= 256, fits, SC_GEMM_G8_MIN < 2^40: the 256 x 192 form;
 *   gemm256     N % 256 == 0, M >= 2048, t256 >= 128 (SC_GEMM_T256_MIN) and t256 >= 85 % (SC_GEMM_FILL_PCT) of its rounds of 256:
 *               gemm256_kernel, one workgroup per tile.  With the default thresholds every such shape is a gemm8p shape: it is
 *               reached only with SC_GEMM_G8_MIN raised or where `fits` fails;
 *   t64         t128 < 384 (SC_GEMM_T128_MIN): gemm_bf16_kernel with 64 x 64 tiles, one workgroup per tile;
 *   persist     N % 8 == 0: gemm_bf16_persist_kernel, 512 resident workgroups walk the 128 x 128 tiles.  With rem = M % 128:
 *               rem != 0, N % 32 == 0, K % 256 == 0 and the ragged row tile would open another round of 512 (SC_GEMM_PEEL=0: never)
 *               -> the last rem rows are a `thin` tail; else rem == 0, t128 > 512 and a last round less than 25 % (SC_GEMM_TAIL_PCT)
 *               full -> the row tiles of that round are a `t64` tail;
 *   t128        everything else (N % 8 != 0): gemm_bf16_kernel with 128 x 128 tiles, one workgroup per tile.
 *   thin = gemm_thin_kernel: one workgroup per 32 x 32 block, sixteen waves split K, added in wave order.
 * The SC_GEMM_* overrides are read from the environment once per process.                                */
int sc_gemm_bf16(int epi, const uint16_t* A, const uint16_t* Wt, const float* bias, void* out, int M, int N, int K, void* stream);
/* The plan sc_gemm_bf16 / sc_gemm_f16 and the tower follow for (epi, M, N, K): host only, launches nothing.  cus: compute units the
 * gemm8p tail rule counts with; cus <= 0 asks the current device (only where the shape reaches that rule).  plan[5] (host memory) =
 * { main kernel (0 t64, 1 t128, 2 persist, 3 gemm8p, 4 gemm8p_192, 5 gemm256), rows of the main kernel, tail kernel (0 none, 1 thin,
 * 2 t64), rows of the tail, tiles of the main kernel }.  Refuses what the GEMM refuses.                     */
int sc_gemm_plan(int epi, int M, int N, int K, int cus, int* plan);
int sc_f32_to_bf16(const float* x, uint16_t* y, long long n, void* stream);
/* The same three entry points with IEEE fp16 operands instead of bf16 (16-bit images / activations are fp16 bit patterns, fp32
 * accumulation, LayerNorm / softmax statistics / residual stream in fp32): the arithmetic the reference's dependency uses on a GPU --
 * clip.load("ViT-L/14", device="cuda") keeps weights and activations in fp16 with fp32 LayerNorm (CLIP_anno.py:16,166-167).  Default
 * of shapeclipper_amd.model.clip_vit.ClipVisionTower since round 3.                                          */
int sc_clip_vit_forward_f16(const float* image, int B, int C, int H, int W, int patch, int D, int mlp, int layers,
                            int heads, int proj_dim, const uint16_t* w_f16, const float* w_f32, float ln_eps,
                            float* out, void* workspace, long long workspace_bytes, void* stream);
int sc_gemm_f16(int epi, const uint16_t* A, const uint16_t* Wt, const float* bias, void* out, int M, int N, int K, void* stream);
int sc_f32_to_f16(const float* x, uint16_t* y, long long n, void* stream);
/* Two stages of the tower on their own (for tests: the tower launches them through the same code).
 * sc_clip_attention: qkv [B*T][3D] 16-bit values (q | k | v; fp16 != 0: IEEE fp16 bit patterns, else bf16), head dim 64 ->
 *   out [B*T][D] = softmax(0.125 q k^T) v per image and head, same 16-bit type.  hipErrorInvalidValue where the tower refuses:
 *   D % 64 != 0, D / heads != 64, a V^T tile over 160 KiB (branches: above).
 * sc_clip_layernorm: rows of D floats, `stride` floats apart (ln_post: stride = T*D reads the class token of every image) ->
 *   out [rows][D] = (x - mean) / sqrt(var + eps) * gamma + beta as fp32 (out16 == 0; out may be x when stride == D, as ln_pre does),
 *   bf16 (1) or fp16 (2).                                                                              */
int sc_clip_attention(const uint16_t* qkv, uint16_t* out, int B, int T, int D, int heads, int fp16, void* stream);
int sc_clip_layernorm(const float* x, int stride, const float* gamma, const float* beta, void* out,
                      int rows, int D, float eps, int out16 /*0: fp32, 1: bf16, 2: fp16*/, void* stream);
/* Small-batch form of the ViT-B layers (csrc/clip_cluster.hpp; same call site, CLIP_anno.py:166-167, at the batch the annotator
 * uses): all transformer layers in ONE launch, an image per cluster of 8 CUs of one XCD, four bounded cluster barriers per layer, no
 * chip-wide synchronisation.  It reads the layer matrices from a RE-PACKED image (same values, the order its waves consume them in: every
 * MFMA fragment one contiguous KB) that sc_clip_cluster_pack builds once per model from the row-major image above.
 * sc_clip_cluster_supported: 1 for width 768 / MLP 3072 / 12 heads / at most 64 tokens per image, else 0.
 * sc_clip_cluster_pack_elems: 16-bit values of the re-packed image (layers * 12 * 768 * 768).
 * sc_clip_cluster_pack: w16 = the tower's 16-bit image (bf16 or fp16 alike), Kp as above, out = the re-packed layers.
 * sc_clip_vit_forward_packed: sc_clip_vit_forward (fp16 == 0) / sc_clip_vit_forward_f16 (fp16 != 0) with w_cluster beside w16; batches of
 * min_b <= B <= max_b images (default 26..32, where it is the faster form; sc_clip_cluster_set_batch_range, or SC_CLIP_CLUSTER_MIN_B / _MAX_B
 * in the environment at load time) on a device with >= 256 CUs take the cluster form, everything else the launch-per-operation form
 * (w_cluster may be NULL then).  A device that cannot hold the grid at once ends every wait after 0.2 s and returns NaN embeddings.       */
int sc_clip_cluster_supported(int D, int mlp, int heads, int tokens);
int sc_clip_cluster_set_batch_range(int min_b, int max_b);
long long sc_clip_cluster_pack_elems(int layers);
int sc_clip_cluster_pack(const uint16_t* w16, int Kp, int layers, uint16_t* out, void* stream);
int sc_clip_vit_forward_packed(const float* image, int B, int C, int H, int W, int patch, int D, int mlp, int layers, int heads,
                               int proj_dim, const uint16_t* w16, const float* w_f32, const uint16_t* w_cluster, int fp16,
                               float ln_eps, float* out, void* workspace, long long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ray sampling (UniformSampler.get_z_vals + point generation, model/renderer.py:13-37,84-86).
 * cam_loc, ray_dirs [n_rays][3]; scale_dist [n_images]; u [n_rays][64] stratified jitter in [0,1) or NULL
 * (evaluation: plain linspace).  Outputs z_vals [n_rays][64], points [n_rays*64][3].  Arithmetic follows the
 * reference's fp32 op order (no fma contraction) so z_vals / points are bit-identical to the torch ops.   */
int sc_ray_sample_forward(const float* cam_loc, const float* ray_dirs, const float* scale_dist, const float* u,
                          int n_rays, int rays_per_image, int n_images, float cam_dist, float* z_vals,
                          float* points, void* stream);
/* adjoint: g_points [P][3] (+ g_z_extra [n_rays][64] from the compositing, may be NULL) -> g_cam_loc,
 * g_ray_dirs [n_rays][3], g_scale_dist [n_rays]: per-RAY contribution; d/d scale_dist[b] is its sum over the
 * rays of image b (left to the caller: one tiny reduction instead of 16K contended atomics).            */
int sc_ray_sample_backward(const float* ray_dirs, const float* z_vals, const float* g_points,
                           const float* g_z_extra, int n_rays, int rays_per_image, int n_images, float cam_dist,
                           float* g_cam_loc, float* g_ray_dirs, float* g_scale_dist, void* stream);
/* The same pair with the eikonal sample points of a training render (model/renderer.py:154-165) produced / differentiated on the way:
 * eik_points [n_images][2 rays_per_image][3] = per image the rays_per_image uniform points (eik_uniform [n_rays][3], copied) followed by the
 * near-surface point of every ray = its sample eik_idx[ray] (int64 [n_rays]; cam_loc + z_eik ray_dir, bit-identical to that entry of
 * `points`).  backward: g_eik_points (may be NULL) adds the near points' gradients to the samples they are; g_points may be NULL (zeros).
 * n_rays == n_images * rays_per_image.                                                                                              */
int sc_ray_sample_forward_eik(const float* cam_loc, const float* ray_dirs, const float* scale_dist, const float* u, const long long* eik_idx,
                              const float* eik_uniform, int n_rays, int rays_per_image, int n_images, float cam_dist, float* z_vals,
                              float* points, float* eik_points, void* stream);
int sc_ray_sample_backward_eik(const float* ray_dirs, const float* z_vals, const float* g_points, const float* g_z_extra, const long long* eik_idx,
                               const float* g_eik_points, int n_rays, int rays_per_image, int n_images, float cam_dist, float* g_cam_loc,
                               float* g_ray_dirs, float* g_scale_dist, void* stream);

/* The sampler pair at S samples per ray (SC_N_SAMPLES_SUPPORTED): u, z_vals, g_z_extra [n_rays][S], points [n_rays*S][3],
 * eik_idx in [0, S).  Bit-identical to the torch op sequence of UniformSampler.get_z_vals at every S.                      */
int sc_ray_sample_forward_ns(const float* cam_loc, const float* ray_dirs, const float* scale_dist, const float* u,
                             int n_rays, int n_samples, int rays_per_image, int n_images, float cam_dist, float* z_vals,
                             float* points, void* stream);
int sc_ray_sample_backward_ns(const float* ray_dirs, const float* z_vals, const float* g_points,
                              const float* g_z_extra, int n_rays, int n_samples, int rays_per_image, int n_images, float cam_dist,
                              float* g_cam_loc, float* g_ray_dirs, float* g_scale_dist, void* stream);
int sc_ray_sample_forward_eik_ns(const float* cam_loc, const float* ray_dirs, const float* scale_dist, const float* u, const long long* eik_idx,
                                 const float* eik_uniform, int n_rays, int n_samples, int rays_per_image, int n_images, float cam_dist,
                                 float* z_vals, float* points, float* eik_points, void* stream);
int sc_ray_sample_backward_eik_ns(const float* ray_dirs, const float* z_vals, const float* g_points, const float* g_z_extra,
                                  const long long* eik_idx, const float* g_eik_points, int n_rays, int n_samples, int rays_per_image,
                                  int n_images, float cam_dist, float* g_cam_loc, float* g_ray_dirs, float* g_scale_dist, void* stream);

/* One render in a single call (Renderer.forward, model/renderer.py:57-152), at 64 samples per ray (sc_render_forward and
 * sc_render_backward take no sample count; other S go through the _ns entry points one by one):
 * sc_ray_sample_forward -> sc_sdf_forward -> sc_rgb_composite_forward.  z_vals, points, sdf, grad, feat and
 * scratch are caller-provided work buffers (sizes as in the three entry points).  Inference: stash_a = stash_p =
 * rgb_flat = NULL.  Training: pass stash_a (5 x TBL64), stash_p (4 x TBL64) and rgb_flat [P][3]; together with
 * z_vals / points / sdf / grad / feat they are what sc_render_backward needs (scratch may then be NULL).    */
/* (sc_render_forward chains sc_ray_sample_forward, sc_sdf_forward and sc_rgb_composite_forward -- the fp32-MFMA forms; the round-6 split
 *  forms sc_sdf_forward_stream / sc_rgb_composite_forward_split are what the Python host calls one by one.)                          */
int sc_render_forward(const float* cam_loc, const float* ray_dirs, const float* depth_fac, const float* scale_dist,
                      const float* u, const float* sdf_pack, const float* sdf_cbias, const float* rgb_pack,
                      const float* rgb_dbias, const float* beta_param, int n_rays, int rays_per_image, int n_images,
                      int symmetric, float cam_dist, float beta_min, float bgcolor, float normal_pow,
                      float* rgb, float* mask, float* mask_hard, float* depth, float* normal,
                      float* z_vals, float* points, float* sdf, float* grad, float* feat, float* scratch,
                      float* stash_a, float* stash_p, float* rgb_flat, void* stream);

/* The whole reverse pass of one training render (what autograd does for model/renderer.py:57-185 and the MLPs of
 * model/implicit.py:138-239, incl. the double backward through d sdf/dx): sc_rgb_composite_backward, the RGB
 * weight-gradient GEMMs, sc_sdf_backward, the SDF weight-gradient GEMMs and sc_ray_sample_backward in one call.
 * Inputs: the forward's operands and saved tensors (see sc_render_forward) and the upstream gradients of the per-ray
 * outputs G_rgb [n_rays][3], G_mask, G_depth [n_rays], G_normal [n_rays][3] (NULL = zero), G_z_extra [n_rays][64]
 * (extra gradient on z_vals, e.g. from the eikonal near-surface samples; may be NULL).
 * Outputs (all fully written): g_sdf_pack [SC_SDF_PACK_FLOATS], g_cbias [5][n_images][64], g_rgb_pack
 * [SC_RGB_PACK_FLOATS], g_dbias [3][n_images][64], g_beta [1], and per ray g_cam_loc [.][3], g_ray_dirs [.][3],
 * g_scale_dist [.] (sum over the rays of an image = d/d scale_dist), g_depth_fac [.].
 * workspace: sc_render_backward_workspace_bytes(n_rays) bytes of device memory (~17 TBL64 tensors).          */
long long sc_render_backward_workspace_bytes(int n_rays);
int sc_render_backward(
    const float* ray_dirs, const float* depth_fac, const float* sdf_pack, const float* rgb_pack, const float* rgb_dbias,
    const float* beta_param, const float* z_vals, const float* points, const float* sdf, const float* grad, const float* feat,
    const float* stash_a, const float* stash_p, const float* rgb_flat, int n_rays, int rays_per_image, int n_images,
    int symmetric, float cam_dist, float beta_min, float bgcolor, float normal_pow,
    const float* G_rgb, const float* G_mask, const float* G_depth, const float* G_normal, const float* G_z_extra,
    float* g_sdf_pack, float* g_cbias, float* g_rgb_pack, float* g_dbias, float* g_beta,
    float* g_cam_loc, float* g_ray_dirs, float* g_scale_dist, float* g_depth_fac,
    void* workspace, long long workspace_bytes, void* stream);

/* compute_level_grid (utils/eval_3D.py:9-38): SDF on linspace(lo,hi,n_axis)^3 ('ij' order) for every image.
 * points_ws: [n_images*n_axis^3][3] floats of workspace; level: [n_images][n_axis][n_axis][n_axis].       */
int sc_sdf_grid_forward(const float* sdf_pack, const float* sdf_cbias, float lo, float hi, int n_axis, int n_images,
                        int symmetric, float* points_ws, float* level, void* stream);
/* round 6: the same grid through the value-only chain in the exact three-piece bf16 split arithmetic with the weights pre-split in LDS
 * (csrc/sdf_value_split.hip: six piece products per fp32 product on v_mfma_f32_16x16x32_bf16, fp32 accumulation -- the arithmetic of the
 * trunk convolutions; error against float64 that of the fp32 chain).  sc_sdf_value_forward_split: the same chain on given points
 * (operands as sc_sdf_forward; sdf [n_points] is the only output).                                                                       */
int sc_sdf_grid_forward_split(const float* sdf_pack, const float* sdf_cbias, float lo, float hi, int n_axis, int n_images,
                              int symmetric, float* points_ws, float* level, void* stream);
int sc_sdf_value_forward_split(const float* points, const float* w_pack, const float* cbias, int n_points, int n_per_image,
                               int n_images, int symmetric, float* sdf, void* stream);
/* round 6: sc_sdf_forward (value, feature, d sdf/dx, training stashes: same operands and outputs) in the same split arithmetic with the
 * pre-split weight fragments STREAMED through LDS one layer at a time (csrc/sdf_fwd_stream.hip: 324 KiB of fragments incl. the transposed
 * set of the adjoint sweep; the 8 waves of a workgroup walk the chain in lock step, two LDS buffers).
 *   sc_sdf_stream_pack_bytes()      bytes of the streamed image (331,776)
 *   sc_sdf_stream_pack              w_pack (fp32 SdfPack image) -> the streamed image; once per weight update
 *   sc_sdf_forward_stream           grad required; stash_a, stash_p and feat all given = the training render (else per-wave `scratch`
 *                                   as in sc_sdf_forward); w_pack is read for the fp32 sdf row of the output layer and its biases      */
long long sc_sdf_stream_pack_bytes(void);
int sc_sdf_stream_pack(const float* w_pack, void* w_stream, void* stream);
int sc_sdf_forward_stream(const float* points, const void* w_stream, const float* w_pack, const float* cbias, int n_points,
                          int n_per_image, int n_images, int symmetric, float* sdf, float* grad, float* feat,
                          float* stash_a, float* stash_p, float* scratch, void* stream);

/* Workgroup-cooperative reverse pass of the SDF MLP (csrc/sdf_bwdw.hip): what sc_sdf_backward + the eight sc_wgrad launches
 * + sc_tbl_sum of the SDF network do, in ONE launch and without the Ga/Gp/r0 hand-off tensors (chain waves and
 * weight-gradient waves of a workgroup exchange operands through LDS).  Requires g_grad and stash_p (the d sdf/dx output
 * is differentiated: every training render) and n_per_image % 16 == 0.
 *   park     workspace, sc_sdf_backward_fused_parts(n_points) * 4 * 4 * 1024 floats (per-wave scratch, stays in L2)
 *   partial  [sc_sdf_backward_fused_parts(n_points)][S], S = sc_sdf_backward_fused_partial_floats(n_images): one partial image
 *            per workgroup, fully written: SdfPack floats of d/d(w_pack) followed (n_images <= 256) by [n_images][5][64] of
 *            d/d(per-image biases); sum them with sc_partial_reduce(partial, parts, S, S, out) -- a fixed summation order
 *   g_cbias  only for n_images > 256 (S == SdfPack floats): [n_images][5][64], zero-filled by the caller, float atomicAdd;
 *            ignored (may be NULL) otherwise
 *   g_points [n_points][3] or NULL.                                                                              */
int sc_sdf_backward_fused_parts(int n_points);
int sc_sdf_backward_fused_partial_floats(int n_images);
int sc_sdf_backward_fused(const float* points, const float* w_pack, int n_points, int n_per_image, int n_images,
                          int symmetric, const float* stash_a, const float* stash_p, const float* g_sdf,
                          const float* g_grad, const float* g_feat, float* g_points, float* park, float* partial,
                          float* g_cbias, void* stream);

/* backward of sc_loss_fused_forward: scales the stored gradients in place by the upstream dL/dloss_k (G4[4],
 * device memory).  g_eik and g_normal_t (n_normal elements, scaled by G4[2]) may be NULL.              */
int sc_loss_fused_backward(const float* G4, float* g_rgb, long long n_rgb, float* g_mask, long long n_mask,
                           float* g_normal, long long n_normal, float* g_eik, long long n_eik, float* g_normal_t,
                           void* stream);

/* ---- encoder glue: BatchNorm2d fused with the residual add / ReLU / stem max-pool around it --------
 * Replaces, between the MIOpen convolutions of the reference's torchvision ResNet-18/34 (model/graph.py:52-54,
 * model/view_estimator.py:40-42; torchvision BasicBlock.forward), nn.BatchNorm2d + `out += identity` + ReLU.
 * All tensors NCHW fp32, contiguous, 16-byte aligned.  N images, C channels, HW = H*W.
 * sc_bn_splits: number S of per-channel partial blocks the kernels use for one group.                       */
int sc_bn_splits(int N, int C);

/* y = [relu]( gamma*(x-mean)*rstd + beta [+ res] ).  training != 0: batch statistics (biased variance), running
 * statistics updated with `momentum` (unbiased variance) and *n_tracked += groups (both may be NULL); training == 0:
 * the running statistics are used.  groups = G >= 1 (N % G == 0): the batch is G independent sub-batches of N/G
 * images (what the reference feeds through the network in G consecutive calls): statistics per sub-batch, running
 * statistics updated G times in order.  save_mean / save_rstd [G][C] are written for the backward.
 * `partial` must hold 2*(2048 + C*G) floats.                                                                  */
int sc_bn_act_forward(const float* x, const float* res, const float* gamma, const float* beta, float* y,
                      float* save_mean, float* save_rstd, float* run_mean, float* run_var, int64_t* n_tracked,
                      float* partial, int N, int C, int HW, int relu, int training, int groups, float eps,
                      float momentum, void* stream);

/* Backward of sc_bn_act_forward.  y (the forward output) is needed only when a residual was added AND relu != 0
 * (pass NULL otherwise: the ReLU mask is then recomputed from x).  dres (may be NULL) receives the gradient of the
 * residual input (= the ReLU-masked dy); dx may be NULL; dgamma / dbeta [C] are always written.               */
int sc_bn_act_backward(const float* dy, const float* x, const float* y, const float* gamma, const float* beta,
                       const float* mean, const float* rstd, float* partial, float* dx, float* dres, float* dgamma,
                       float* dbeta, int N, int C, int HW, int relu, int training, int groups, void* stream);

/* ResNet stem: y = maxpool3x3/stride2/pad1( relu( bn(x) ) ), x [N,C,H,W] -> y [N,C,Ho,Wo], Ho = (H-1)/2+1.
 * idx [N,C,Ho,Wo] int32: argmax position h*W+w (first maximum in scan order, as torch.nn.MaxPool2d).          */
int sc_bn_relu_pool_forward(const float* x, const float* gamma, const float* beta, float* y, int* idx,
                            float* save_mean, float* save_rstd, float* run_mean, float* run_var, int64_t* n_tracked,
                            float* partial, int N, int C, int H, int W, int training, int groups, float eps,
                            float momentum, void* stream);
int sc_bn_relu_pool_backward(const float* dy, const int* idx, const float* x, const float* gamma, const float* beta,
                             const float* mean, const float* rstd, float* partial, float* dx, float* dgamma,
                             float* dbeta, int N, int C, int H, int W, int training, int groups, void* stream);

/* ---- iso-surface extraction for evaluation (replaces mcubes.marching_cubes, utils/eval_3D.py:125) -----
 * level [n_images][n_axis]^3 fp32.  sc_isosurface_count writes counts[cube] (cube = ((b*Nc + x)*Nc + y)*Nc + z,
 * Nc = n_axis-1): number of triangles of the marching-tetrahedra surface {level = iso} inside the cube (0..12).
 * The caller turns counts into exclusive offsets (int64 prefix sum) and allocates tris [total][3][3];
 * sc_isosurface_emit writes the triangles of every cube at its offset, vertices in grid-index units.           */
int sc_isosurface_count(const float* level, int n_images, int n_axis, float iso, int* counts, void* stream);
int sc_isosurface_emit(const float* level, int n_images, int n_axis, float iso, const int* counts,
                       const long long* offsets, float* tris, void* stream);

/* sc_marching_cubes_*: the same contract with marching CUBES (the algorithm of the reference's PyMCubes call, utils/eval_3D.py:
 * 123-153): up to 5 triangles per cube from the 256-case table of csrc/mc_table.hpp (generated by tools/gen_mc_table.py).  The
 * vertex set is the one every marching-cubes implementation produces -- one vertex per grid edge whose end values lie on
 * different sides of iso (inside = value < iso), at the linear interpolation point -- the triangulation of ambiguous faces
 * (diagonal corners inside) cuts off the inside corners, identically on both sides of the face.                          */
int sc_marching_cubes_count(const float* level, int n_images, int n_axis, float iso, int* counts, void* stream);
int sc_marching_cubes_emit(const float* level, int n_images, int n_axis, float iso, const int* counts,
                           const long long* offsets, float* tris, void* stream);

/* Block form of both (what the Python side uses): a workgroup owns 1,024 consecutive cubes of one image.
 *   sc_isosurface_blocks_per_image(n_axis)   blocks per image = ceil((n_axis-1)^3 / 1024)  (-1: n_axis outside 2..1024)
 *   *_block_count    block_counts [n_images * blocks_per_image] int: triangles of each block
 *   sc_isosurface_block_scan   (round 6) block_offsets [n_images * blocks_per_image + 1] = exclusive int64 prefix sum of block_counts with
 *                    the total as its last entry, per_image [n_images] = triangles of each image: one launch of one workgroup between
 *                    the two passes (the caller reads per_image to size `tris`).
 *   *_block_emit     block_offsets: that array (n_images * blocks_per_image + 1 entries: a block whose neighbours' offsets are equal holds
 *                    no triangle and is left at once); the kernel recomputes the per-cube counts and takes
 *                    their prefix inside the workgroup -- no per-cube count / offset arrays (12 bytes per cube), and the prefix sum
 *                    between the launches runs over 1/1024 of the values.  Same triangles in the same order as the per-cube form. */
int sc_isosurface_blocks_per_image(int n_axis);
int sc_isosurface_block_scan(const int* block_counts, int n_images, int n_axis, long long* block_offsets, long long* per_image, void* stream);
int sc_isosurface_block_count(const float* level, int n_images, int n_axis, float iso, int* block_counts, void* stream);
int sc_isosurface_block_emit(const float* level, int n_images, int n_axis, float iso, const long long* block_offsets, float* tris,
                             void* stream);
int sc_marching_cubes_block_count(const float* level, int n_images, int n_axis, float iso, int* block_counts, void* stream);
int sc_marching_cubes_block_emit(const float* level, int n_images, int n_axis, float iso, const long long* block_offsets, float* tris,
                                 void* stream);
/* round 6, what the Python side runs for marching cubes: the count pass also leaves the case index of every cube (masks
 * [n_images * (n_axis-1)^3] bytes, caller-allocated), the emit pass reads them instead of re-reading 8 corners per cube and deals the
 * vertices of a 256-cube group out to all lanes (coalesced 12-byte stores).  Same triangles, same order, bit for bit.                   */
int sc_marching_cubes_block_count_masks(const float* level, int n_images, int n_axis, float iso, int* block_counts, unsigned char* masks,
                                        void* stream);
int sc_marching_cubes_block_emit_masks(const float* level, int n_images, int n_axis, float iso, const long long* block_offsets,
                                       const unsigned char* masks, float* tris, void* stream);

/* Indexed marching-cubes mesh (what ops.isosurface_mesh runs; the reference's `mcubes.marching_cubes` returns this form).  Vertices: one
 * per grid edge (p, p + e_axis) whose end values lie on different sides of iso (inside = value < iso), owned by its lower end p =
 * (x, y, z), axis 0/1/2 = +x/+y/+z; per image ordered by the linear index (x*n_axis + y)*n_axis + z of p, then by axis; position in
 * grid-index units, the soup's interpolation of the same edge bit for bit.  Faces: triangle f of image b is triangle f of the soup of
 * sc_marching_cubes_block_count_masks / _emit_masks for image b, same corner order, as int32 vertex numbers LOCAL to the image.
 *   sc_marching_cubes_mesh_vertex_blocks_per_image(n_axis)   ceil(n_axis^3 / 1024) workgroups of grid points per image (-1: n_axis
 *                    outside 2..1024)
 *   sc_marching_cubes_mesh_vertex_count   block_counts [n_images * vertex blocks per image] int: crossing edges owned by each block
 *   sc_marching_cubes_mesh_vertex_scan    block_offsets [n_images * vertex blocks per image + 1] int64 exclusive prefix (total last) and
 *                    per_image [n_images] vertices of each image, as sc_isosurface_block_scan.  The caller reads per_image, sizes verts
 *                    [total][3] and must refuse an image with more than 2^31 - 1 vertices (its numbers would not fit int32).
 *   sc_marching_cubes_mesh_vertex_emit    verts at those offsets; vmap [n_images][n_axis^3][3] int32 (caller-allocated, no fill needed:
 *                    written at crossing edges only) receives each crossing edge's image-local vertex number.
 *   sc_marching_cubes_mesh_face_emit      faces [triangles][3] int32 at the soup's offsets: block_offsets and masks are the soup's cube
 *                    scan and case indices (sc_isosurface_block_scan over sc_marching_cubes_block_count_masks), vmap the array above.
 * Scratch: vmap 12 bytes per grid point (396 MB for 32 images at n_axis 101, 1.6 GB for one at 513), masks 1 byte per cube, 4 + 8
 * bytes per 1,024-point or 1,024-cube block.                                                                                              */
int sc_marching_cubes_mesh_vertex_blocks_per_image(int n_axis);
int sc_marching_cubes_mesh_vertex_count(const float* level, int n_images, int n_axis, float iso, int* block_counts, void* stream);
int sc_marching_cubes_mesh_vertex_scan(const int* block_counts, int n_images, int n_axis, long long* block_offsets, long long* per_image,
                                       void* stream);
int sc_marching_cubes_mesh_vertex_emit(const float* level, int n_images, int n_axis, float iso, const long long* block_offsets, float* verts,
                                       int* vmap, void* stream);
int sc_marching_cubes_mesh_face_emit(int n_images, int n_axis, const long long* block_offsets, const unsigned char* masks, const int* vmap,
                                     int* faces, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dual contouring of the level grid (csrc/dual_contour.hip; what ops.dual_contour_mesh runs).  It works on the state of the indexed
 * marching-cubes mesh above -- masks (the case byte of every cube, sc_marching_cubes_block_count_masks), verts and vmap
 * (sc_marching_cubes_mesh_vertex_emit), vertex_block_offsets (sc_marching_cubes_mesh_vertex_scan) -- plus normals [vertices][3] fp32, one
 * per crossing vertex in the order of verts.  A crossing vertex with its normal is Hermite data (p_i, n_i).  "Inside" is value < iso, the
 * rule that wrote masks; a NaN is outside.  Corner v of a cube is its lower corner + (v & 1, (v >> 1) & 1, (v >> 2) & 1).
 *
 * Cells.  A cell is a cube of 8 grid points with lower corner g = (x, y, z), 0 <= x, y, z <= n_axis - 2.  It owns one dual vertex iff its
 * case byte is neither 0 nor 255; an image's dual vertices are numbered in ascending linear cell index (x (n_axis-1) + y)(n_axis-1) + z.
 * The cell reads its crossings through vmap in the order of its 12 edges e = 0..11 = (corner, corner): (0,1) (0,2) (0,4) (1,3) (1,5)
 * (2,3) (2,6) (3,7) (4,5) (4,6) (5,7) (6,7); edge e is a crossing iff its corners' bits of the case byte differ.  All arithmetic is
 * fp32, every operation rounded once (no contraction), every comparison a true comparison (false when an operand is NaN):
 *   s = (0,0,0), k = 0;  for e ascending, crossings only:  s_j = s_j + p_e,j (j = 0, 1, 2),  k = k + 1
 *   c_j = s_j / (float)k
 *   a00 = a01 = a02 = a11 = a12 = a22 = 0, b = (0,0,0);  for e ascending, crossings whose three normal components all have
 *   |n_j| <= FLT_MAX only (a normal with a NaN or Inf component counts for c and k and for nothing else), n = n_e:
 *       d_j = p_e,j - c_j;   w = (n_0 d_0 + n_1 d_1) + n_2 d_2;   a_ij = a_ij + n_i n_j  (i <= j);   b_j = b_j + n_j w
 *   r = reg * (float)k;   a00 = a00 + r,  a11 = a11 + r,  a22 = a22 + r          -- (sum n n^T + reg k I) y = sum n (n . (p - c))
 *   LDL^T, divisions only:   l10 = a01 / a00;   l20 = a02 / a00;   e1 = a11 - l10 a01;   t21 = a12 - l20 a01;   l21 = t21 / e1;
 *       e2 = (a22 - l20 a02) - l21 t21;   z1 = b_1 - l10 b_0;   z2 = (b_2 - l20 b_0) - l21 z1;
 *       y_2 = z2 / e2;   y_1 = z1 / e1 - l21 y_2;   y_0 = (b_0 / a00 - l10 y_1) - l20 y_2
 *   x_j = c_j + y_j;   if !(x_j >= (float)g_j) then x_j = (float)g_j;   if !(x_j <= (float)(g_j + 1)) then x_j = (float)(g_j + 1)
 * so every dual vertex lies in its own cell's unit box, and a NaN (from a NaN level value at an end of a crossing) lands on g_j.
 * With reg > 0 the matrix is positive definite: a00 >= r > 0, and e1, e2 > 0 up to rounding.
 *
 * Faces.  One quad, as two triangles, per crossing grid edge that has four cells around it: for the edge from grid point P along axis
 * a with (a, b, c) a cyclic permutation of (x, y, z), both P_b and P_c lie in 1..n_axis-2 (edges on the faces of the grid emit nothing:
 * the surface is open there, as the marching-cubes surface is).  Its cells, all at P_a along a, are q0 = (P_b - 1, P_c - 1),
 * q1 = (P_b, P_c - 1), q2 = (P_b, P_c), q3 = (P_b - 1, P_c); the triangles are (q0, q1, q2), (q0, q2, q3) when P is inside (the quad's
 * normal then points along +a, out of the solid, the orientation of the marching-cubes faces) and (q0, q2, q1), (q0, q3, q2) otherwise.
 * Faces are ordered by owning edge -- image, linear index of P, axis: the order of the crossing vertices -- and hold int32 dual vertex
 * numbers LOCAL to the image.
 *   sc_dual_contour_count      cell_block_counts, face_block_counts [n_images * sc_isosurface_blocks_per_image(n_axis)] int: owning
 *                    cells and triangles (2 per quad) of every block of 1,024 consecutive cubes; sc_isosurface_block_scan turns each
 *                    into int64 offsets and per-image totals.  The caller reads the totals and sizes dual_verts [cells][3] and faces
 *                    [triangles][3] (a cell count fits int32 because a cube count does).
 *   sc_dual_contour_cell_emit  dual_verts at the cell offsets; cell_map [n_images][(n_axis-1)^3] int32 (caller-allocated, no fill
 *                    needed: written at owning cells only) receives each owning cell's image-local dual vertex number.
 *   sc_dual_contour_face_emit  faces at the face offsets, from masks and cell_map.
 * Plain vector stores, no atomics: the same bits from run to run, whatever n_images or the stream.  n_images <= 0 returns 0 and launches
 * nothing; hipErrorInvalidValue for n_axis outside [2, 1024], a NULL pointer, or a reg that is not a finite number > 0.               */
int sc_dual_contour_count(const unsigned char* masks, int n_images, int n_axis, int* cell_block_counts, int* face_block_counts, void* stream);
int sc_dual_contour_cell_emit(const unsigned char* masks, const float* verts, const float* normals, const int* vmap,
                              const long long* vertex_block_offsets, int n_images, int n_axis, float reg, const long long* cell_block_offsets,
                              float* dual_verts, int* cell_map, void* stream);
int sc_dual_contour_face_emit(const unsigned char* masks, const int* cell_map, int n_images, int n_axis, const long long* face_block_offsets,
                              int* faces, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Similarity ICP of the evaluation (csrc/icp.hip; what ops.icp_fit / icp_apply / icp_align run).  The search between two fits is
 * sc_chamfer3d_forward* above; these are the fit, the apply and the objective around it.  src [n_images][n][3] and dst [n_images][m][3]
 * fp32; idx1 [n_images][n] int32 = nearest dst point of each CURRENT (transformed) source point, idx2 [n_images][m] int32 = nearest
 * current source point of each dst point, as sc_chamfer3d_forward* writes them.  transform [n_images][4][4] and scale [n_images] float64.
 * The file is built without contraction: every operation below rounds once, in float64 unless it says fp32.
 *
 * Pairs.  Image b has two halves of pairs (p, q), p always an ORIGINAL source point (the fit is absolute, not incremental):
 *   half 1: (src[i], dst[idx1[i]]) for i = 0..n-1, weight 1/n each;   half 2: (src[idx2[j]], dst[j]) for j = 0..m-1, weight 1/m each.
 * An index outside its cloud turns the pair into NaNs (no read out of bounds); the image then keeps its previous transform.
 *
 * Sums.  For a per-pair term f, <f> = (S1(f) / n + S2(f) / m) / 2, S1 and S2 the sums of f over the two halves: the weight is applied to
 * the half's sum, not to each term (so equal points average to themselves exactly).  Each half is cut into chunks of SC_ICP_CHUNK =
 * 1,024 consecutive pairs, one workgroup of 256 threads per chunk, and a half's sum is formed in this order:
 *   thread t adds its chunk's pairs t, t + 256, t + 512, t + 768, ascending (pairs past the end of the half add nothing);
 *   each wave folds its 64 lanes by v += v[lane + 32], then + 16, + 8, + 4, + 2, + 1; the workgroup adds its four wave sums in wave order;
 *   the chunk partials are added in ascending chunk number.
 * No float atomics anywhere: partials are plain stores, read by a later launch.  The same bits from run to run, on any stream, and for an
 * image whatever else is in the batch.
 *
 * sc_icp_fit (Umeyama): pm = <p>, qm = <q>; with dp = p - pm, dq = q - qm:  H = <dq dp^T> (H_rc = <dq_r dp_c>),
 *   var_p = <(dp_0 dp_0 + dp_1 dp_1) + dp_2 dp_2>.  H = U D V^T by one-sided Jacobi in one thread per image: A = H, V = I; sweeps over the
 *   column pairs (0,1), (0,2), (1,2) rotate A's and V's columns from the right until every pair of A's columns is orthogonal to 1e-16 of
 *   the product of their norms (at most 30 sweeps); D = the column norms, sorted descending with the columns, u_k = a_k / d_k.
 *   R = U diag(1, 1, det U det V) V^T, formed as u_0 v_0^T + u_1 v_1^T + (u_0 x u_1)(v_0 x v_1)^T (the same matrix, and defined when
 *   d_2 = 0);  s = ((d_0 + d_1) + sigma d_2) / var_p with sigma = det U det V = sign((a_2 . (u_0 x u_1)) (v_2 . (v_0 x v_1))), or s = 1
 *   when with_scale == 0;  M = s R;  t_r = qm_r - ((M_r0 pm_0 + M_r1 pm_1) + M_r2 pm_2).
 *   transform = [M t; 0 0 0 1], scale = s.  The image keeps its previous transform and scale -- prev_transform / prev_scale, both NULL
 *   for the identity and 1; they may be transform / scale themselves -- when a sum is not finite, var_p <= 0, d_1 <= 1e-12 d_0 (rank
 *   <= 1: the rotation is undetermined), or s or an entry of M or t is not finite.  Three launches: means per chunk, centred sums per
 *   chunk (each workgroup first adds the mean partials in the stated order), solve.
 * sc_icp_apply: out[i][r] = fp32(((M_r0 x + M_r1 y) + M_r2 z) + t_r), (x, y, z) = src[i] widened to float64; one rounding to fp32.
 * sc_icp_objective: objective[b * objective_stride] = S1(dist1) / n + S2(dist2) / m in float64, the sums in the order above (dist1
 *   [n_images][n], dist2 [n_images][m] fp32, the squared distances of the search).  Two launches.
 * workspace: sc_icp_workspace_bytes(n_images, n, m) bytes (128 per chunk), contents irrelevant on entry; fit and objective may share it
 *   on one stream.  -1 for sizes the entry points refuse.
 * n_images <= 0 returns 0 and launches nothing; hipErrorInvalidValue for a NULL pointer (prev_* aside, which must be NULL together),
 * n or m < 1, n_images > 65535 or objective_stride < 1.                                                                                */
#define SC_ICP_CHUNK 1024
long long sc_icp_workspace_bytes(int n_images, int n, int m);
int sc_icp_fit(const float* src, const float* dst, const int* idx1, const int* idx2, int n_images, int n, int m, int with_scale,
               const double* prev_transform, const double* prev_scale, double* workspace, double* transform, double* scale, void* stream);
int sc_icp_apply(const float* src, const double* transform, int n_images, int n, float* out, void* stream);
int sc_icp_objective(const float* dist1, const float* dist2, int n_images, int n, int m, double* workspace, double* objective,
                     long long objective_stride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * k nearest neighbours inside a cloud, PCA normals from them, normal consistency of two clouds (csrc/point_normals.hip; what
 * ops.knn_points / point_normals / normal_consistency run; the evaluation's --eval.normals).  The file is built without contraction:
 * every operation below rounds once; tests/point_normals_ref.py restates all of it in numpy.
 *
 * sc_knn_points: points [n_images][n][3] fp32 -> idx [n_images][n][k] int32, dist [n_images][n][k] fp32.  For point i and every point j
 *   of the same image (j = i included, as Open3D and PCL count it):
 *       dx = p_j,0 - p_i,0, dy, dz likewise;   d = (dx dx + dy dy) + dz dz   in fp32 (five roundings; not Chamfer's fmaf form);
 *       key = (bits(d) << 32) | j   as an unsigned 64-bit integer, bits(d) the 32 bits of the fp32 value.
 *   Row i holds the k smallest keys in ascending order: idx = the low word, dist = the value whose bits are the high word.  d >= +0 or
 *   NaN, so the unsigned order of the bits is the numeric order and a NaN sorts last; the keys of a row are distinct, so the order is
 *   total: ties go to the lower index, duplicates need no rule, and the result is unique whatever order the search meets candidates in.
 *   Search: a uniform grid over the cloud's bounding box (integer atomics only; arbitrary order inside a cell), the queries taken in
 *   cell order, Chebyshev rings of cells around the query's cell.  After ring r every unseen point is at least lb away along one
 *   axis; the walk stops when the list is full and  kth d < (lb - slack)^2 * 0.9999,  slack = 16 * 2^-23 * (max |coordinate| + largest
 *   extent) for the rounding of the binning and of the faces, the factor for the rounding of d: no unseen point can beat or tie the
 *   k-th key.  A query that has not stopped after 4 rings or 4,096 candidates, and every query of an image with a coordinate that is
 *   not finite or >= 1e15 in magnitude, is answered by a scan of ALL points with the same key.  (SC_KNN_FORCE_SCAN=1 in the
 *   environment, read once, sends every query to the scan: a timing aid.)
 *   workspace: sc_knn_workspace_bytes(n_images, n, k) bytes, contents irrelevant on entry; -1 for sizes sc_knn_points refuses.
 * sc_point_normals: points and idx [n_images][n][k] (any k indices per point; sc_knn_points' rows in rank order) -> normals
 *   [n_images][n][3] fp32, variation [n_images][n] fp32.  Float64 throughout, q_r = points[idx[i][r]] widened (an index outside
 *   0..n-1 counts as a NaN point, no read out of bounds):
 *       m_a = (sum_r q_r,a) / k, r ascending from 0;    d_r = q_r - m;    C_ab = (sum_r d_r,a d_r,b) / k, r ascending (a <= b).
 *   Eigenvectors by the cyclic two-sided Jacobi method, V = I, exactly 8 sweeps over the pairs (p, q) = (0,1), (0,2), (1,2), r the
 *   third index.  A rotation is skipped when C_pq == 0; otherwise
 *       theta = (C_qq - C_pp) / (2 C_pq);   t = sgn(theta) / (|theta| + sqrt(theta theta + 1))  (sgn(0) = 1),  or  t = 0.5 / theta
 *       when |theta| > 1e150 (where theta theta overflows);   c = 1 / sqrt(t t + 1);   s = t c;   h = t C_pq;
 *       C_pp = C_pp - h;  C_qq = C_qq + h;  C_pq = 0;  (C_rp, C_rq) = (c C_rp - s C_rq,  s C_rp + c C_rq);
 *       (V_ip, V_iq) = (c V_ip - s V_iq,  s V_ip + c V_iq)  for i = 0, 1, 2.
 *   The diagonal sorted ascending (equal values keep their index order) is l0 <= l1 <= l2.  The normal is V's column of l0, negated
 *   when its component of largest magnitude (the first one on a tie) is negative, then rounded once to fp32: unoriented but
 *   deterministic.  variation = fp32(l0 / ((l0 + l1) + l2)).  A point is degenerate -- normal (0,0,0), variation 0 -- when a component
 *   of m or C or an eigenvalue is not finite, or when l1 <= 1e-12 l2 (rank <= 1: collinear or coincident neighbours, no plane).
 * sc_normal_consistency: n1 [n_images][n][3], n2 [n_images][m][3] fp32, idx1 [n_images][n], idx2 [n_images][m] int32 (as
 *   sc_chamfer3d_forward* writes them for the two clouds) -> acc, comp [n_images] float64:
 *       acc[b] = S1(|n1[i] . n2[idx1[i]]|) / n,    comp[b] = S2(|n2[j] . n1[idx2[j]]|) / m,    u . v = (u_0 v_0 + u_1 v_1) + u_2 v_2
 *   on values widened to float64; S1 and S2 are formed exactly in the order stated for sc_icp_objective above (chunks of SC_ICP_CHUNK,
 *   thread, wave, workgroup, chunk stages; no float atomics).  An index outside its cloud contributes NaN (no read out of bounds), so
 *   that image's value is NaN and the other images' are untouched.  workspace: 8 bytes per chunk of either half
 *   (sc_icp_workspace_bytes(n_images, n, m) is more than enough), contents irrelevant on entry.
 * Plain stores and integer atomics only: the same bits from run to run, on any stream, and for an image whatever else is in the batch.
 * n_images <= 0 returns 0 and launches nothing; hipErrorInvalidValue for a NULL pointer, k outside 3..32, n < k (n, m < 1 for
 * sc_normal_consistency) or n_images > 65535.                                                                                           */
long long sc_knn_workspace_bytes(int n_images, int n, int k);
int sc_knn_points(const float* points, int n_images, int n, int k, void* workspace, int* idx, float* dist, void* stream);
int sc_point_normals(const float* points, const int* idx, int n_images, int n, int k, float* normals, float* variation, void* stream);
int sc_normal_consistency(const float* n1, const float* n2, const int* idx1, const int* idx2, int n_images, int n, int m,
                          double* workspace, double* acc, double* comp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exact distance from points to a triangle mesh (csrc/point_mesh.hip; what ops.point_mesh_distance runs; the evaluation's
 * --eval.mesh_dist).  The file is built without contraction: every operation below is fp32 and rounds once, every comparison is a true
 * comparison (false when an operand is NaN); tests/point_mesh_ref.py restates all of it in numpy.
 *
 * points [n_images][n_points][3] fp32; verts [v_total][3] fp32 and faces [f_total][3] int32, the images' meshes packed one after the
 * other; v_count, f_count [n_images] int32 on the device: image b owns the next v_count[b] vertices and f_count[b] faces (negative
 * counts read as 0, nothing is read past v_total / f_total).  Face indices are LOCAL to the image's vertex slice, as
 * sc_isosurface_mesh_* and sc_dual_contour_* write them; a face with an index outside [0, v_count[b]) is skipped (no read out of
 * bounds).  -> dist2 [n_images][n_points] fp32 (squared distance), face [n_images][n_points] int32 (local index of the winning
 * triangle), closest [n_images][n_points][3] fp32 (the closest point on it).
 *
 * Arithmetic of one pair, point p against triangle (a, b, c) -- the region walk of Ericson, Real-Time Collision Detection 5.1.5:
 *       u . v = (u_0 v_0 + u_1 v_1) + u_2 v_2;      ab = b - a;  ac = c - a;  bc = c - b;  ap = p - a;  bp = p - b;  cp = p - c;
 *       d1 = ab . ap;  d2 = ac . ap;  d3 = ab . bp;  d4 = ac . bp;  d5 = ab . cp;  d6 = ac . cp;
 *       vc = d1 d4 - d3 d2;   vb = d5 d2 - d1 d6;   va = d3 d6 - d5 d4;   e1 = d4 - d3;   e2 = d5 - d6.
 *   The first region whose test holds gives the closest point q:
 *       vertex A:  d1 <= 0 and d2 <= 0:                                      q = a
 *       vertex B:  d3 >= 0 and d4 <= d3:                                     q = b
 *       edge AB:   vc <= 0 and d1 >= 0 and d3 <= 0 and d1 - d3 > 0:          v = d1 / (d1 - d3);          q = a + v ab
 *       vertex C:  d6 >= 0 and d5 <= d6:                                     q = c
 *       edge AC:   vb <= 0 and d2 >= 0 and d6 <= 0 and d2 - d6 > 0:          w = d2 / (d2 - d6);          q = a + w ac
 *       edge BC:   va <= 0 and e1 >= 0 and e2 >= 0 and e1 + e2 > 0:          w = e1 / (e1 + e2);          q = b + w bc
 *       interior:  den = (va + vb) + vc > 0 and va >= 0, vb >= 0, vc >= 0 and den > 1e-5f * ((ab . ab) * (ac . ac)):
 *                                                                            v = vb / den;  w = vc / den;  q = (a + v ab) + w ac
 *   (the "> 0" of the edge tests keeps 0 / 0 out: a == b leaves edge AB to the tests behind it; the signs asked of the interior keep
 *   v and w in [0, 1], so every region returns a point within a few ulp of the triangle, which the search's stopping rule relies on;
 *   den is |ab|^2 |ac|^2 sin^2 of the angle at a: below sin^2 = 1e-5 the weights are quotients of rounding noise and the triangle,
 *   thinner than 0.0032 of its length, is taken as its edges by the rule below, an error of at most its width).
 *   If no region claims the point -- a thin triangle, or rounding on one of zero area -- q is the first minimum, in the order AB, AC,
 *   BC, over the clamped closest points of the three segments: for a segment from s along e,  l = e . e;  t = ((p - s) . e) / l;
 *   t = 0 unless l > 0;  t = 0 unless t >= 0;  t = 1 if t > 1;  q = s + t e;  AB's candidate is taken first, AC's and then BC's replace
 *   it when their distance is strictly smaller.  In every case  d = (p - q) . (p - q).  a == b == c acts as a point, a collinear triangle as a
 *   segment; a finite query against finite vertices below 2^29 in magnitude (no product overflows) never yields NaN.
 *   A triangle with a vertex that is not finite is tested like any other: no region claims the pair (every comparison with NaN is
 *   false) and the segment rule decides, so it counts through an edge whose two ends are finite, if it has one.
 * Winner: a candidate (d, f) replaces the best so far when  d < best || (d == best && f < best_f),  from best = +Inf, best_f = INT_MAX:
 *   the lowest face index among the exact minima -- a query on a shared vertex or edge ties exactly -- whatever order the candidates are
 *   met in, and a NaN distance never wins.  An image without a winner (f_count == 0, or only skipped faces) gets dist2 = +Inf,
 *   face = -1, closest = 0;  a query with a coordinate that is not finite gets dist2 = NaN, face = -1, closest = NaN, and every other
 *   row is untouched by it.
 * sc_point_mesh_distance_brute tests all pairs (triangles staged through LDS, the query in registers).  sc_point_mesh_distance gives the
 *   same bits from an exact grid search in the manner of sc_chamfer3d_forward_grid: a uniform grid over the bounding box of the image's
 *   valid triangles, cell side max(2 x the mean of the triangles' largest AABB extents, cbrt(box volume / faces)) grown until the grid
 *   has at most 2 faces + 64 cells; a triangle is referenced from every cell its AABB, padded by slack, overlaps (count pass, exclusive
 *   scan, fill pass; integer atomics, arbitrary order inside a cell), or, when that is more than 16 cells, from the image's "large" list,
 *   which every query of the image tests -- so the references fit 16 f_total slots whatever the mesh and nothing is read back to the
 *   host.  A query (one thread each) walks Chebyshev rings of cells around its own cell, clamped into the grid.  After ring r no unseen
 *   triangle has a point inside the (2r+1)^3 block, so all of it is at least lb away, lb the distance to the nearest block face that
 *   is not a face of the grid; the walk stops when  best < (lb - slack)^2 * 0.9999,  slack = 16 * 2^-23 * (max |coordinate| + largest
 *   extent), or when the block covers the grid.  A query that has not stopped after 6 rings or 4,096 candidates, or that lies more than
 *   two cells outside the box, goes on a list, as does every query of an image whose grid is unusable (a referenced vertex that is not
 *   finite or >= 1e15 in magnitude, a box of zero extent); the list is answered by the all-pairs loop, 16 slices of the faces merged
 *   with 64-bit atomicMin on (bits of d) << 32 | face, the winner's closest point recomputed by the pair arithmetic.
 * Plain vector stores and integer atomics only: the same bits from run to run, on any stream, for an image alone or in a batch.
 * workspace: sc_point_mesh_workspace_bytes(n_images, n_points, v_total, f_total) bytes for either entry point, 16-byte aligned,
 *   contents irrelevant on entry; 0 for n_images <= 0, -1 for sizes the entry points refuse.  n_images <= 0 returns 0 and launches
 *   nothing; hipErrorInvalidValue for n_images > 65535, n_points < 1, n_images * n_points > 2^30, v_total < 0, f_total outside
 *   [0, 2^26], a NULL pointer (verts / faces may be NULL when their total is 0) or a misaligned workspace.                          */
long long sc_point_mesh_workspace_bytes(int n_images, int n_points, int v_total, int f_total);
int sc_point_mesh_distance(const float* points, const float* verts, const int32_t* faces, const int32_t* v_count, const int32_t* f_count,
                           int n_images, int n_points, int v_total, int f_total, void* workspace, float* dist2, int32_t* face,
                           float* closest, void* stream);
int sc_point_mesh_distance_brute(const float* points, const float* verts, const int32_t* faces, const int32_t* v_count,
                                 const int32_t* f_count, int n_images, int n_points, int v_total, int f_total, void* workspace,
                                 float* dist2, int32_t* face, float* closest, void* stream);

/* ---- evaluation: Earth Mover's Distance of two equal-sized clouds by an auction matching (csrc/emd3d.hip) -----------------------
 * sc_emd3d_match finds, per image, a bijection phi of the persons xyz1 [n_images][n][3] onto the objects xyz2 [n_images][n][3] (fp32,
 * 2 <= n <= SC_EMD3D_MAX_POINTS) that minimises  sum_i |xyz1_i - xyz2_phi(i)|  (Euclidean, not squared) to within n eps, by Bertsekas'
 * forward auction in its Jacobi form with epsilon scaling, and reports the mean cost of its pairs.  tests/emd_ref.py restates the
 * rule below in numpy and the outputs match it bit for bit.
 *
 * Cost of person i = (ax, ay, az) and object j = (bx, by, bz), fp32, one rounding per operation (built without contraction):
 *       dx = ax - bx;  dy = ay - by;  dz = az - bz;  d2 = (dx dx + dy dy) + dz dz;  c_ij = sqrt(d2), correctly rounded.
 *   It is recomputed by this expression wherever it is needed.
 * Phases: eps_list [n_eps] fp32 on the HOST (copied into the launch; 1 <= n_eps <= SC_EMD3D_MAX_PHASES, every entry finite and > 0)
 *   holds the epsilon of every phase.  ops.emd_match computes it in fp32:  e = eps_start;  while e > eps: emit e, e = fl(e / 4);  then
 *   emit eps  (0.25 and 1e-4 give 7 phases).  Prices p_j are zero before the first phase and kept from phase to phase; at the start of a
 *   phase every person is unassigned and every object unowned.
 * Round: a pure function of the state at its start.  Every person i that is unassigned at the start of the round bids, against the
 *   prices at the start of the round:
 *       w_j = fl(fl(-c_ij) - p_j) for every object j;   j* = the lowest j among the maxima of w, w1 = w_j*;   w2 = max of w_j over j != j*;
 *       b = fl(p_j* + fl(fl(w1 - w2) + e)).
 *   Object j goes to the highest b bid for it, among equal b to the lowest person index -- the maximum of the 64-bit integer key
 *   (bits(b) << 32) | (0xFFFFFFFF - i), b > 0 so bit order is value order: the winner becomes its owner, the previous owner becomes
 *   unassigned, p_j = b.  A bidder that wins nothing stays unassigned.
 * A phase ends when nobody is unassigned; the auction has converged when the last phase has ended.  rounds counts the rounds of all
 *   phases.  Before every round, if rounds >= max_rounds (>= 1) the auction stops where it is with converged = 0 (an auction that ends
 *   in exactly max_rounds rounds has converged), so the kernel ends under every input; the bijection is then completed: the persons
 *   still unassigned, in ascending index, take the objects still unowned, in ascending index.
 * -> assignment [n_images][n] int32 (phi), cost [n_images][n] fp32 (c_i,phi(i)), price [n_images][n] fp32 (p_j of every object),
 *   rounds, converged [n_images] int32, emd [n_images] float64 = (cost[0] + cost[1] + ... in ascending i, added in float64 by one
 *   lane) / n.  For a converged auction every person's pair is within eps of its best at the final prices (epsilon-complementary
 *   slackness, up to the fp32 roundings of a bid), hence  optimum <= emd <= optimum + eps.
 * An image with a coordinate that is not finite is detected before the first round: assignment = identity, cost = price = 0,
 *   rounds = 0, converged = 0, emd = NaN; the other images of the batch are untouched by it.  Finite coordinates so large that a cost
 *   overflows (above about 1e19) give an unspecified bijection; indices stay in bounds and max_rounds still ends the auction.
 * Launch: ONE workgroup of 1024 threads per image, the whole auction inside it with workgroup barriers only --
 *   no wait on another workgroup, no host read, no float atomics.  A wave takes one bidder at a time, its lanes striding over the
 *   objects; the bids of a round meet in one 64-bit integer LDS max per bidder.  Dynamic LDS 48 n bytes: key 8, object position 12,
 *   price 4, owner 4, object of a person 4, list of the unassigned 4, person position 12 -- 96 KiB at n = 2048 of the CU's 160 KiB,
 *   above the 64 KiB default, so the launch raises the kernel's dynamic-LDS limit first.
 * The rounds are Jacobi and the winner rule does not depend on the order bids arrive in: the same bits from run to run, on any stream,
 *   for an image alone or in a batch.  No workspace.  n_images <= 0 returns 0 and launches nothing; hipErrorInvalidValue for
 *   n_images > 65535, n outside [2, SC_EMD3D_MAX_POINTS], n_eps outside [1, SC_EMD3D_MAX_PHASES], an epsilon that is not finite and
 *   positive, max_rounds < 1 or a NULL pointer.                                                                                      */
#define SC_EMD3D_MAX_POINTS 2048
#define SC_EMD3D_MAX_PHASES 80
int sc_emd3d_match(const float* xyz1, const float* xyz2, int n_images, int n, const float* eps_list, int n_eps, int max_rounds,
                   int32_t* assignment, float* cost, float* price, int32_t* rounds, int32_t* converged, double* emd, void* stream);

/* ---- evaluation: volumetric IoU of two point clouds from voxel solids (csrc/voxel_solid.hip) -------------------------------------
 * A cloud becomes a solid of an R^3 grid (SC_VOXEL_MIN_RES <= R <= SC_VOXEL_MAX_RES): its points are splatted to a voxel shell, the
 * shell is closed by c dilations (0 <= c <= SC_VOXEL_MAX_CLOSE), the space the exterior cannot reach is filled, and the result is
 * eroded c times.  Two clouds share one frame and the IoU is that of their solids.  tests/voxel_iou_ref.py restates every step in
 * numpy and all outputs match it bit for bit.  fp32 below is un-fused, one rounding per operation (built without contraction).
 *
 * sc_voxel_frame: the frame of a pair of clouds a [n_images][n_a][3], b [n_images][n_b][3] (fp32; n_a, n_b >= 1), m = c + 1:
 *       lo = min over both clouds, hi = max over both clouds, per axis;   side = max(max(hi_x - lo_x, hi_y - lo_y), hi_z - lo_z);
 *       pitch = side / float(R - 2 m),  pitch = 1.0f when side == 0;   centre = (lo + hi) * 0.5f;
 *       origin = centre - (R * 0.5f) * pitch     per axis.
 *   The object fills the cube up to m empty layers on every side: a dilation never reaches the border and the exterior is connected
 *   around the object.  If any coordinate of either cloud is not finite, origin and pitch are the quiet NaN 0x7fc00000; finite
 *   coordinates whose differences or sums overflow give the Inf or NaN of the expressions above.
 *   -> origin [n_images][3], pitch [n_images] fp32.  One workgroup of 1024 threads per image; minima and maxima do not depend on order.
 *
 * sc_voxel_solid: points [n_images][n][3] fp32 (n >= 1), origin [n_images][3], pitch [n_images] (any frame, usually sc_voxel_frame's).
 *   Storage: one 64-bit word per (x, y) row, bit z: a volume is R^2 words, bit z of word x R + y is voxel (x, y, z).
 *   Shell: for every point p with three finite coordinates, per axis
 *       q = (p - origin) / pitch  (a true division);   i = int(min(max(floorf(q), float(m)), float(R - 1 - m)))
 *     (the clamp is made in fp32, so a q beyond the integers is defined: it is  clamp(int(floorf(q)), m, R - 1 - m)  wherever that
 *     is), and voxel (i_x, i_y, i_z) is set.  A point with a coordinate that is not finite sets nothing; with an origin or a pitch
 *     that is not finite, or pitch <= 0, no point sets anything.
 *   Solid:  D = the shell dilated c times by the 3x3x3 cube.   Exterior E = the least set that holds the border voxels (x, y or z
 *     equal to 0 or R - 1) not in D and, with a voxel, its 6-neighbours not in D.   F = not E.   Solid = F eroded c times by the cube,
 *     the outside of the grid counting as empty --  binary_erosion(binary_fill_holes(binary_dilation(shell, cube, c)), cube, c)  of
 *     scipy.ndimage.  E is a unique fixed point: no schedule of the flood changes a bit of it.
 *   The flood runs Jacobi sweeps until one changes nothing: with `free` = the voxels of a row not in D,
 *       v = (E[x][y] | E[x-1][y] | E[x+1][y] | E[x][y-1] | E[x][y+1]) & free     (rows outside the grid are empty),
 *       E'[x][y] = v smeared along z inside `free` until it stops growing,
 *     from  E[x][y] = free  on the border rows (x or y equal to 0 or R - 1) and  free & (bit 0 | bit R - 1)  elsewhere.  sweeps
 *     counts every sweep, the last, which changes nothing, included.
 *   -> bits [n_images][R][R] int64 (the solid), shell_voxels, solid_voxels, sweeps [n_images] int32.
 *   Launch: ONE workgroup of 1024 threads per image, the whole job in LDS with workgroup barriers only: no wait on another
 *   workgroup, no spin on global memory, no host read; the sweep loop ends because E only grows in a finite grid.  Points are
 *   splatted by a 64-bit integer LDS OR; dilation and erosion are separable (shifts inside a word along z, neighbouring words along
 *   y and x); every reduction is an integer sum.  Dynamic LDS 24 R^2 bytes (three volumes: 96 KiB at R = 64 of the CU's 160 KiB,
 *   above the 64 KiB default, so the launch raises the kernel's dynamic-LDS limit first).
 *
 * sc_voxel_iou: bits_a, bits_b [n_images][words] int64 -> inter [n_images] = popcount of the AND, uni [n_images] = popcount of the
 *   OR, int32 (words <= 2^24, so they cannot overflow).  One workgroup of 256 threads per image.  The IoU is inter / uni in float64,
 *   1 for an empty union (ops.mask_iou's convention) -- left to the caller.
 *
 * No float atomics anywhere: the same bits from run to run, on any stream, for an image alone or in a batch.  No workspace.
 * n_images <= 0 returns 0 and launches nothing; hipErrorInvalidValue for n_images > 65535, a count < 1, res or close out of range,
 * words outside [1, 2^24] or a NULL pointer.                                                                                          */
#define SC_VOXEL_MIN_RES 8
#define SC_VOXEL_MAX_RES 64
#define SC_VOXEL_MAX_CLOSE 2
int sc_voxel_frame(const float* a, const float* b, int n_images, int n_a, int n_b, int res, int close, float* origin, float* pitch,
                   void* stream);
int sc_voxel_solid(const float* points, const float* origin, const float* pitch, int n_images, int n, int res, int close, int64_t* bits,
                   int32_t* shell_voxels, int32_t* solid_voxels, int32_t* sweeps, void* stream);
int sc_voxel_iou(const int64_t* bits_a, const int64_t* bits_b, int n_images, int words, int32_t* inter, int32_t* uni, void* stream);

/* ---- evaluation: topology, area and volume of indexed triangle meshes (csrc/mesh_topology.hip) ----------------------------------------
 * A batch of meshes packed one after the other, the form of the sc_marching_cubes_mesh_* and sc_dual_contour_* entry points:
 * verts [n_verts][3] fp32, faces [n_faces][3] int32 with vertex numbers LOCAL to their image, v_off / f_off [n_images + 1] int64 the
 * running sums of the per-image counts (v_off[0] = f_off[0] = 0, v_off[n_images] = n_verts, f_off[n_images] = n_faces, ascending).
 * Image b sees only verts[v_off[b] : v_off[b+1]] and faces[f_off[b] : f_off[b+1]]; everything below is per image, and face numbers
 * are local to the image as well.  tests/mesh_topology_ref.py restates every rule in numpy.
 *
 * Faces.  A face with an index outside [0, v_off[b+1] - v_off[b]) sets *bad_index to 1, is never dereferenced and takes part in
 *   nothing (the caller raises; the other outputs of the call are then unspecified).  A face with two equal indices is DEGENERATE:
 *   it is counted in degenerate_faces and takes part in nothing else.
 * Edges.  An undirected edge is {a, b} of consecutive indices (i0,i1), (i1,i2), (i2,i0) of a non-degenerate face; the face traverses
 *   it FORWARD when it lists min(a,b) before max(a,b) in that cyclic order.  Per edge: count = the faces on it (two faces with the same
 *   three indices are two faces), fwd = how many of them traverse it forward, minface = the lowest face number on it.
 * Components.  Classes of the non-degenerate faces under "share an undirected edge" (every face of an edge is united with the edge's
 *   minface).  face_component [n_faces] int32 = the lowest local face number of the face's class; -1 for a face that takes no part.
 * Corners.  A corner is a (face, vertex) pair of a non-degenerate face.  For every edge {a, b} and every face f on it, corner (f, a) is
 *   united with (minface, a) and (f, b) with (minface, b).  The FANS of a vertex are the corner classes at it; a vertex with more
 *   than one fan is non-manifold (a pinch point, or two boundary chains that meet in a point).
 * counts [SC_MESH_TOPOLOGY_FIELDS][n_images] int64, row by row:
 *    0 vertices               referenced by a non-degenerate face        1 unreferenced_vertices  the others
 *    2 faces                  non-degenerate                             3 degenerate_faces
 *    4 edges                  distinct undirected edges                  5 boundary_edges         count == 1
 *    6 nonmanifold_edges      count >= 3                                 7 inconsistent_edges     count == 2 and fwd != 1
 *    8 components                                                        9 largest_component_faces
 *   10 nonmanifold_vertices   more than one fan                         11 euler = vertices - edges + faces
 *   12 genus = components - euler / 2 when rows 13, 14, 15 are all 1 and faces > 0 (euler is even then), else -1
 *   13 watertight = boundary_edges == 0 && nonmanifold_edges == 0       14 oriented = inconsistent_edges == 0
 *   15 manifold = nonmanifold_edges == 0 && nonmanifold_vertices == 0
 *   An image without faces gets zeros (unreferenced_vertices = its vertices), genus -1 and the three flags 1.
 * area, volume [n_images] float64.  Per non-degenerate face with vertices p0, p1, p2 widened exactly to float64, every operation
 *   rounded once (the file is built without contraction; sqrt and the division are the correctly rounded ones):
 *       e1 = p1 - p0, e2 = p2 - p0;   n = (e1_y e2_z - e1_z e2_y,  e1_z e2_x - e1_x e2_z,  e1_x e2_y - e1_y e2_x);
 *       area term   = sqrt((n_x n_x + n_y n_y) + n_z n_z) * 0.5;
 *       c = (p1_y p2_z - p1_z p2_y,  p1_z p2_x - p1_x p2_z,  p1_x p2_y - p1_y p2_x);
 *       volume term = ((p0_x c_x + p0_y c_y) + p0_z c_z) / 6.0      (signed; meaningful for a watertight, oriented mesh).
 *   A face that takes no part has the terms +0.0.  Order of the sums: an image's faces are cut into chunks of SC_MESH_TOPOLOGY_CHUNK =
 *   256 consecutive faces from its first face; a chunk's partial is 0.0 plus its terms in ascending face number, one addition at a
 *   time; the image's sum is 0.0 plus the chunk partials in ascending chunk number.  Partials are plain stores read by a later
 *   launch: no float atomics, and the order does not depend on the launch shape, the batch or the stream.
 * Edge table.  Open addressing in scratch, table_slots slots: a power of two, > 3 n_faces (so every linear probe meets an empty or
 *   matching slot) and <= 2^30.  The key (global lo << 32) | global hi over image-offset vertex numbers is claimed by a 64-bit
 *   compare-and-swap on the empty key; count and fwd by integer adds, minface by an integer min.  The two union-finds hook by an
 *   integer min onto a smaller label, so every find loop walks strictly decreasing labels and ends whatever other threads do.  Only
 *   integer atomics decide integer outputs: no output depends on arrival order or on table_slots.
 * Seven launches on `stream` (three when n_faces == 0), no wait on another workgroup, no host synchronisation.  scratch:
 * sc_mesh_topology_scratch_bytes(n_images, n_verts, n_faces, table_slots) bytes of device memory, 16-byte aligned, contents irrelevant
 * on entry (the query gives 0 for sizes the entry point refuses).  n_images <= 0 returns 0 and launches nothing;
 * hipErrorInvalidValue for n_images > 65535, n_faces > 2^26, a negative count, a table_slots that is not such a power of two, a NULL
 * pointer or a misaligned scratch (verts may be NULL when n_verts == 0, faces and face_component when n_faces == 0).                     */
#define SC_MESH_TOPOLOGY_CHUNK 256
#define SC_MESH_TOPOLOGY_FIELDS 16
long long sc_mesh_topology_scratch_bytes(int n_images, int n_verts, int n_faces, int table_slots);
int sc_mesh_topology(const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images, int n_verts,
                     int n_faces, int table_slots, void* scratch, int64_t* counts, double* area, double* volume, int32_t* face_component,
                     int32_t* bad_index, void* stream);

/* ---- evaluation: decimation by vertex clustering with quadric placement (csrc/mesh_simplify.hip) -------------------------------------
 * What ops.mesh_cluster_simplify runs and {idx}_mesh_simplified.ply holds (`--eval.simplify`).  A batch of packed meshes in the form of
 * sc_mesh_topology above (verts, faces with image-local indices, v_off / f_off).  A box of `cells` = G cells per axis (1 <= G <=
 * SC_MESH_SIMPLIFY_MAX_CELLS = 128, so G^3 <= 2^21), each of side `pitch` = h > 0, with its lower corner at origin = o (three fp32
 * values, like h widened exactly to float64), is laid over every image; all vertices of an image that fall into one cell (Rossignac and
 * Borrel) become ONE vertex, placed by the cell's quadric (Lindstrom).  tests/mesh_simplify_ref.py restates every rule in numpy.  All
 * arithmetic is float64, every operation rounded once (the file is built without contraction; the divisions are correctly rounded).
 *
 * Vertices.  p = the vertex widened exactly to float64;  q_j = (p_j - o_j) / h  (j = 0, 1, 2).  A vertex with a p_j that is not finite
 *   or a q_j outside [0, G] sets *bad_vertex to 1, gets vertex_cluster -1 and takes part in nothing, and neither does a face that holds
 *   it (the caller raises; the other outputs of the call are then unspecified).  Otherwise its cell is g_j = min(floor(q_j), G - 1) (a
 *   vertex on the upper face of the box belongs to the last cell), its cell id (g_0 G + g_1) G + g_2, and u_j = q_j - (g_j + 0.5).
 * Clusters.  The clusters of an image are its occupied cells, numbered from 0 in ascending cell id (a bit per cell in a mask, an integer
 *   block scan over the mask's popcounts).  vertex_cluster [n_verts] int32 = the cluster number of every vertex, local to the image.
 * Accumulators, SC_MESH_SIMPLIFY_ACC = 13 per cluster, all int64, fed by 64-bit integer atomic adds only:
 *   n += 1 and s_j += llrint(u_j 2^24) for every vertex of the cluster (round to nearest, ties to even; |u_j| <= 0.5, so |s_j| <= 2^54);
 *   a face TAKES PART if its three indices lie in [0, v_off[b+1] - v_off[b]) -- else it sets *bad_index to 1 and is never
 *   dereferenced -- and are pairwise distinct.  With a, b, c its corners in the order it lists them:
 *       e1 = q_b - q_a,  e2 = q_c - q_a;   N = (e1_1 e2_2 - e1_2 e2_1,  e1_2 e2_0 - e1_0 e2_2,  e1_0 e2_1 - e1_1 e2_0)
 *   and, once for each DISTINCT cluster among the three corners' clusters, with g the cell of that cluster:
 *       w_j = q_a,j - (g_j + 0.5);   d = (N_0 w_0 + N_1 w_1) + N_2 w_2;
 *       A_ij += fix(N_i N_j) for (i,j) = (0,0) (0,1) (0,2) (1,1) (1,2) (2,2);    b_j += fix(N_j d)
 *       fix(t) = llrint(clamp(t, -2^12, 2^12) 2^24)          (t > 2^12 ? 2^12 : t < -2^12 ? -2^12 : t;  the scaling is exact)
 *   N is twice the face's area vector in cell units, so a face that spans more than about 8 cells saturates instead of overflowing.
 *   A face whose three corners fall into ONE cluster still adds its terms there: it carries the plane.  No sum can leave int64:
 *   |fix| <= 2^36 and the entry point refuses more than 2^26 faces, so every |A_ij|, |b_j| <= 2^62.
 * Solve, per cluster.  A_ij, b_j, s_j converted to float64 (round to nearest, ties to even) and scaled by 2^-24 (exact);
 *       c_j = s_j / (double)n;    lam = reg * ((A_00 + A_11) + A_22);
 *   if !(lam > 0) then x = c, else with a00 = A_00 + lam, a11 = A_11 + lam, a22 = A_22 + lam, a01 = A_01, a02 = A_02, a12 = A_12 and
 *   b_j = b_j + lam c_j, the division-only LDL^T of the dual-contouring block above:
 *       l10 = a01 / a00;   l20 = a02 / a00;   e1 = a11 - l10 a01;   t21 = a12 - l20 a01;   l21 = t21 / e1;
 *       e2 = (a22 - l20 a02) - l21 t21;   z1 = b_1 - l10 b_0;   z2 = (b_2 - l20 b_0) - l21 z1;
 *       x_2 = z2 / e2;   x_1 = z1 / e1 - l21 x_2;   x_0 = (b_0 / a00 - l10 x_1) - l20 x_2
 *   which solves (sum N N^T + lam I) x = sum N d + lam c: the point nearest the planes of the cluster's faces, drawn towards the mean
 *   of its vertices.  Then  if !(x_j >= -0.5) x_j = -0.5;  if !(x_j <= 0.5) x_j = 0.5  (a NaN lands on a bound), and
 *       verts_out_j = (float)(o_j + ((g_j + 0.5) + x_j) h)
 *   so every output vertex lies in its own cell.  verts_out is packed image after image in cluster order.  A cluster whose faces all
 *   vanished stays as an unreferenced vertex.
 * Faces.  A face that takes part maps to the cluster numbers (k_a, k_b, k_c) of its corners, keeping its rotation.  It is COLLAPSED, and
 *   dropped, when two of them are equal.  The others are grouped by their unordered triple (an open-addressing table in scratch, image
 *   b owning slots [2 f_off[b] + b, 2 f_off[b+1] + b + 1): more slots than faces, so a linear probe always meets an empty or matching
 *   slot; the key (lo << 42) | (mid << 21) | hi of the ascending triple is claimed by a 64-bit compare-and-swap on the empty key).  A
 *   face is EVEN when (k_a, k_b, k_c) is a rotation of (lo, mid, hi), ODD otherwise.  Per group and parity: the number of faces (integer
 *   add) and the lowest face number (integer min).  A face is WRITTEN iff it is the lowest face of its parity in its group and that
 *   parity has strictly more faces than the other: opposite faces cancel -- a sheet folded onto itself vanishes and the surface stays
 *   closed -- and of several like-oriented copies one stays.  faces_out [.][3] int32 holds the written faces' image-local cluster
 *   triples, packed image after image in ascending source face number (block-scan compaction); face_source [.] int32 their image-local
 *   source face numbers.
 * counts [SC_MESH_SIMPLIFY_FIELDS][n_images] int64, row by row: 0 vertices_out (clusters), 1 faces_out (written faces), 2 collapsed
 *   faces, 3 cancelled faces = the faces that take part, are not collapsed and are not written.
 * The caller allocates verts_out [n_verts][3], faces_out [n_faces][3] and face_source [n_faces] (the outputs cannot be larger) and reads
 * counts to see how much of each was written.  Only integer atomics decide anything: every output has the same bits from run to run,
 * for any batch, stream and face order (the face list follows the source order by definition).  Ten launches on `stream` (six when
 * n_faces == 0), no wait on another workgroup, no host synchronisation.  scratch: sc_mesh_cluster_simplify_scratch_bytes(n_images,
 * n_verts, n_faces, cells) bytes of device memory, 16-byte aligned, contents irrelevant on entry (the query gives 0 for sizes the entry
 * point refuses).  n_images <= 0 returns 0 and launches nothing; hipErrorInvalidValue for n_images > 65535, n_faces > 2^26, a negative
 * count, cells outside 1..128, n_images ceil(cells^3 / 64) > 2^28, an origin, pitch or reg that is not finite, pitch <= 0, reg <= 0, a
 * NULL pointer or a misaligned scratch (verts, verts_out and vertex_cluster may be NULL when n_verts == 0; faces, faces_out and
 * face_source when n_faces == 0).                                                                                                        */
#define SC_MESH_SIMPLIFY_MAX_CELLS 128
#define SC_MESH_SIMPLIFY_ACC 13
#define SC_MESH_SIMPLIFY_FIELDS 4
long long sc_mesh_cluster_simplify_scratch_bytes(int n_images, int n_verts, int n_faces, int cells);
int sc_mesh_cluster_simplify(const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images, int n_verts,
                             int n_faces, float origin_x, float origin_y, float origin_z, float pitch, int cells, double reg, void* scratch,
                             float* verts_out, int32_t* faces_out, int64_t* counts, int32_t* vertex_cluster, int32_t* face_source,
                             int32_t* bad_vertex, int32_t* bad_index, void* stream);

/* ---- post-processing: Taubin lambda|mu smoothing by the umbrella operator (csrc/mesh_smooth.hip) --------------------------------------
 * What ops.mesh_smooth runs and {idx}_mesh_smooth.ply holds (`--mesh.smooth`).  A batch of packed meshes in the form of sc_mesh_topology
 * above (verts, faces with image-local indices, v_off / f_off); everything below is per image.  The faces are not changed, so neither is
 * the topology.  tests/mesh_smooth_ref.py restates every rule in numpy.  All arithmetic is float64, every operation rounded once (the
 * file is built without contraction; sqrt and the divisions are the correctly rounded ones).
 *
 * Faces.  A face with an index outside [0, v_off[b+1] - v_off[b]) sets *bad_index to 1, is never dereferenced and takes part in nothing
 *   (the caller raises; the other outputs of the call are then unspecified).  Every other face, degenerate or not, takes part with its
 *   DISTINCT undirected edges: {a, b} of consecutive corners (i0,i1), (i1,i2), (i2,i0) with a != b, each once per face -- (a, a, b) has
 *   the one edge {a, b}, (a, a, a) none.
 * Edges.  count = the faces that have the edge (two faces with the same three indices are two faces).
 * Neighbours.  N(i) = the distinct vertices j != i that share an edge with i, whatever its count;  |N(i)| is the DEGREE of i.
 * Vertices.  A vertex with a component that is not finite sets *bad_vertex to 1 (the caller raises).  i is FIXED_BOUNDARY if it lies on
 *   an edge of count 1 (the open rim that the grid boundary cuts: it must not creep inward), ISOLATED if N(i) is empty (no face, or only
 *   faces like (i, i, i), names it), FREE otherwise; an edge of count >= 3 is an ordinary edge.  Only free vertices move.
 * State.  x_i = the vertex widened exactly to float64.  A HALF-STEP with factor f maps every free i, per component, to
 *       s = +0.0;  s = s + x_j for j in N(i) in ASCENDING j;   m = s / (double)|N(i)|;   d = m - x_i;   t = f d;   x_i' = x_i + t
 *   reading only the state at its start (Jacobi); the others keep their bits.  One ITERATION is a half-step with lam, then, if mu != 0, a
 *   half-step with mu (Taubin: 0 < lam <= 1, -1 <= mu <= 0; mu = 0 is plain Laplacian smoothing).  `iters` iterations run (0 <= iters <=
 *   SC_MESH_SMOOTH_MAX_ITERS = 1000; 0 returns the input bits).
 * verts_out [n_verts][3] fp32 = the final state rounded to fp32 once (to nearest, ties to even); the input bits for a vertex that is not
 *   free.
 * counts [SC_MESH_SMOOTH_FIELDS][n_images] int64, row by row: 0 free, 1 fixed_boundary, 2 isolated (the three sum to the image's
 *   vertices), 3 degree_max (over all its vertices; 0 without one).
 * measures [SC_MESH_SMOOTH_MEASURES][n_images] float64, row by row, with |v| = sqrt((v_x v_x + v_y v_y) + v_z v_z) and m_i as above:
 *    0 rough_before  the mean over the free vertices of |m_i - x_i| on the start state     1 rough_after  the same on the final state
 *    2 disp_mean     the mean over the free vertices of |x_i(final) - x_i(start)|           3 disp_max     the largest of them
 *   (the final state is the float64 one, before the rounding to fp32).  Order of the sums: an image's vertices are cut into chunks of
 *   SC_MESH_SMOOTH_CHUNK = 256 consecutive vertices from its first vertex; a vertex that is not free has the terms +0.0; a chunk's
 *   partial is 0.0 plus its terms in ascending vertex number, one addition at a time; the image's sum is 0.0 plus the chunk partials in
 *   ascending chunk number; a mean is that sum / (double)free.  disp_max folds the same way with  acc = term > acc ? term : acc  from
 *   0.0.  All four are 0.0 for an image without a free vertex.  Partials are plain stores read by a later launch: no float atomics.
 * Edge table.  Open addressing in scratch, table_slots slots: a power of two, > 3 n_faces (so every linear probe meets an empty or
 *   matching slot) and <= 2^30.  The key (global lo << 32) | global hi over image-offset vertex numbers is claimed by a 64-bit
 *   compare-and-swap on the empty key; the thread that claims a slot adds one to the degree of both ends, every face adds one to the
 *   slot's count (integer adds).  The rows of a CSR adjacency (offsets: an integer block scan of the degrees) are filled at an integer
 *   atomic cursor and then put into ascending order by rank, so the arrival order leaves no trace; there is no cap on the degree.
 *   Only integer atomics decide anything: every output has the same bits from run to run, for any batch, stream, face order and
 *   table_slots.
 * 7 + (mu != 0 ? 2 : 1) iters launches on `stream`, one per half-step, two fewer when n_faces == 0; no wait on another workgroup, no
 * host synchronisation.  scratch: sc_mesh_smooth_scratch_bytes(n_images, n_verts, n_faces, table_slots) bytes of device memory, 16-byte
 * aligned, contents irrelevant on entry (the query gives 0 for sizes the entry point refuses).  n_images <= 0 returns 0 and launches
 * nothing; hipErrorInvalidValue for n_images > 65535, n_faces > 2^26, n_verts > 2^30, a negative count, a table_slots that is not such a
 * power of two, iters outside 0..1000, lam outside (0, 1], mu outside [-1, 0], a NULL pointer or a misaligned scratch (verts and
 * verts_out may be NULL when n_verts == 0, faces when n_faces == 0).                                                                    */
#define SC_MESH_SMOOTH_CHUNK 256
#define SC_MESH_SMOOTH_FIELDS 4
#define SC_MESH_SMOOTH_MEASURES 4
#define SC_MESH_SMOOTH_MAX_ITERS 1000
long long sc_mesh_smooth_scratch_bytes(int n_images, int n_verts, int n_faces, int table_slots);
int sc_mesh_smooth(const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images, int n_verts,
                   int n_faces, int table_slots, int iters, double lam, double mu, void* scratch, float* verts_out, int64_t* counts,
                   double* measures, int32_t* bad_vertex, int32_t* bad_index, void* stream);

/* ---- post-processing: one Loop subdivision step and one Newton step onto the SDF's zero set (csrc/mesh_subdivide.hip) -----------------
 * What ops.mesh_subdivide and ops.mesh_project_step run and {idx}_mesh_subdiv.ply holds (`--mesh.subdivide`).  A batch of packed meshes
 * in the form of sc_mesh_topology above (verts, faces with image-local indices, v_off / f_off); everything below is per image.
 * sc_mesh_subdivide does ONE level: every face becomes four.  tests/mesh_subdivide_ref.py restates every rule in numpy.  The
 * subdivision arithmetic is float64, every operation rounded once (the file is built without contraction).
 *
 * Faces.  A face with an index outside [0, v_off[b+1] - v_off[b]) sets *bad_index to 1 and is never dereferenced; a face in range that
 *   repeats an index sets *bad_face to 1; neither takes part in anything.  A vertex with a component that is not finite sets *bad_vertex
 *   to 1.  The caller raises for each of the three; the other outputs of the call are then unspecified.  No producer of the library
 *   emits a face that repeats an index, and such a face is not repaired here.
 * Half-edges.  Corner c of face f (f counted over the packed faces) is half-edge 3 f + c; its edge runs from i_c to i_{(c+1) % 3}, the
 *   vertex i_{(c+2) % 3} lies opposite.
 * Edges.  The undirected edge {lo, hi} keeps  count = its half-edges (the faces that have it),  owner = the lowest of their numbers,
 *   omin / omax = the lowest / highest opposite vertex number.  An edge is INTERIOR if count == 2 -- omin and omax are then its two
 *   opposite vertices, whatever the winding (the same vertex twice for a doubled face) -- and SHARP otherwise: 1 is the rim that the grid
 *   face cuts, 3 or more is non-manifold.
 * Vertices.  N(i) = the distinct vertices that share an edge with i, n = |N(i)| its DEGREE.  i is FIXED if it lies on a sharp edge,
 *   ISOLATED if it lies on no edge, INTERIOR otherwise.
 * State.  x_i = the input vertex widened exactly to float64; both rules read it and nothing else.
 * Even (old) vertices keep their number.  FIXED and ISOLATED ones keep their bits.  An INTERIOR one becomes, per component,
 *       s = +0.0;  s = s + x_j for j in N(i) in ASCENDING j;   beta = (n == 3) ? 0.1875 : 0.375 / (double)n;
 *       w = (n == 3) ? 0.4375 : 0.625;   a = w x_i;   r = beta s;   x' = a + r          (Loop's scheme with Warren's weights)
 * Odd (new) vertices, one per edge:  e = x_lo + x_hi;  interior:  o = x_omin + x_omax;  a = 0.375 e;  r = 0.125 o;  p = a + r;
 *   sharp:  p = 0.5 e, and the new vertex is FIXED.
 * Numbering.  An edge's vertex is V_b + r, r the rank of the edge among the image's edges in ascending owner (an integer block scan over
 *   the image's 3 F_b flags "this half-edge is its edge's owner"), so the numbering follows the input face order.  Image b's output
 *   vertices are [V_b old | E_b new]; the images' blocks are packed in image order, the offsets taken on the device from the edge counts.
 * verts_out [n_verts + 3 n_faces][3] fp32 (the bound; the first sum of vertices_out rows are used): x' and p rounded to fp32 once (to
 *   nearest, ties to even), the input bits for a vertex that keeps them.  fixed_out [n_verts + 3 n_faces] bytes: 1 for a FIXED vertex,
 *   old or new, else 0.
 * faces_out [4 n_faces][3] image-local: with m_c the vertex of corner c's edge, face f becomes
 *       4 f: (i0, m0, m2)    4 f + 1: (i1, m1, m0)    4 f + 2: (i2, m2, m1)    4 f + 3: (m0, m1, m2)
 *   The winding is kept, so orientation, genus, watertightness and the number of components are kept by construction.
 * counts [SC_MESH_SUBDIVIDE_FIELDS][n_images] int64, row by row: 0 vertices_out = V_b + E_b, 1 edges, 2 sharp_edges, 3 fixed_vertices
 *   (old and new: the fixed old ones plus sharp_edges), 4 isolated, 5 degree_max (over all its vertices; 0 without one).
 * Edge table.  Open addressing in scratch, table_slots slots: a power of two, > 3 n_faces (so every linear probe meets an empty or
 *   matching slot) and <= 2^30.  The key (global lo << 32) | global hi over image-offset vertex numbers is claimed by a 64-bit
 *   compare-and-swap on the empty key; the thread that claims a slot adds one to the degree of both ends; count by an integer add, owner
 *   and omin by atomicMin, omax by atomicMax.  The rows of a CSR adjacency (offsets: an integer block scan of the degrees) are filled at
 *   an integer atomic cursor and then put into ascending order by rank, a wave for a row of more than 32 entries; there is no cap on the
 *   degree.  Only integer atomics decide anything: every output has the same bits from run to run, for any batch, stream and
 *   table_slots; permuting the input faces permutes the output and changes no position's bits.
 * 8 launches on `stream` (5 when n_faces == 0); no wait on another workgroup, no float atomic, no host synchronisation.  scratch:
 * sc_mesh_subdivide_scratch_bytes(n_images, n_verts, n_faces, table_slots) bytes of device memory, 16-byte aligned, contents irrelevant
 * on entry (the query gives 0 for sizes the entry point refuses).  n_images <= 0 returns 0 and launches nothing; hipErrorInvalidValue
 * for n_images > 65535, n_faces > 2^24 (4 n_faces <= 2^26: the output is an input of the next level), n_verts > 2^30, a negative count,
 * a table_slots that is not such a power of two, a NULL pointer or a misaligned scratch (verts may be NULL when n_verts == 0, faces and
 * faces_out when n_faces == 0, verts_out and fixed_out when both are).
 *
 * sc_mesh_project_step: one clamped Newton step of every vertex onto {sdf = 0}; elementwise, fp32, every operation rounded once (the
 * division and the square root are the correctly rounded ones), a thread per vertex.  With f = sdf[i], g = grad[i] (d sdf / d position in
 * the SDF's own units) and v = verts[i]:
 *       g2 = (gx gx + gy gy) + gz gz
 *   v keeps its bits if fixed[i] != 0, if f or g2 is not finite, or if g2 < 1e-12f.  Otherwise
 *       t = f / g2;   d_c = (t g_c) scale;   l = sqrtf((dx dx + dy dy) + dz dz)
 *   v keeps its bits if l is not finite;  if l > max_step:  r = max_step / l;  d_c = d_c r;   then v'_c = v_c - d_c.
 * `scale` turns the SDF's units into those of verts.  n_verts == 0 returns 0 and launches nothing; hipErrorInvalidValue for a negative
 * n_verts, more than 2^30 or a NULL pointer.                                                                                             */
#define SC_MESH_SUBDIVIDE_FIELDS 6
long long sc_mesh_subdivide_scratch_bytes(int n_images, int n_verts, int n_faces, int table_slots);
int sc_mesh_subdivide(const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images, int n_verts,
                      int n_faces, int table_slots, void* scratch, float* verts_out, int32_t* faces_out, uint8_t* fixed_out, int64_t* counts,
                      int32_t* bad_vertex, int32_t* bad_index, int32_t* bad_face, void* stream);
int sc_mesh_project_step(const float* verts, const float* sdf, const float* grad, const uint8_t* fixed, int n_verts, float scale,
                         float max_step, float* verts_out, void* stream);

/* ---- post-processing: one round of quadric edge-collapse decimation towards a face budget (csrc/mesh_decimate.hip) -------------------
 * What ops.mesh_decimate runs and {idx}_mesh_decimated.ply holds (`--mesh.decimate`).  A batch of packed meshes in the form of
 * sc_mesh_topology above (verts, faces with image-local indices, v_off / f_off); everything below is per image.
 * sc_mesh_decimate_round does ONE round, a pure function of the mesh it is given: quadrics are recomputed from the current faces every
 * round ("memoryless" simplification) and nothing but the vertex map `parent` is carried from round to round.  The caller repeats rounds
 * and ends with sc_mesh_decimate_compact.  tests/mesh_decimate_ref.py restates every rule in numpy.  All real arithmetic is float64 from
 * the exactly widened fp32 positions x_i, every operation rounded once (the file is built without contraction), every sum in the stated
 * order; a position is rounded to fp32 once, when it is written.
 *
 * Faces, half-edges, edges (count, owner, omin, omax) and FIXED vertices (on an edge whose count is not 2: the rim that the grid face
 *   cuts, non-manifold spots) are those of sc_mesh_subdivide above, with its three flags: flags[0] a vertex that is not finite, flags[1]
 *   a face index out of range (never dereferenced), flags[2] a face that repeats an index; such faces take part in nothing and the
 *   caller raises.  A fixed vertex is never moved and never removed.  ring(i) = the vertices that share an edge with i, ASCENDING.
 * Triangle terms.  For a vertex v and two others u, w:  N = (x_u - x_v) x (x_w - x_v), each component  a b - c d  with the two products
 *   rounded;  d = (N.x p.x + N.y p.y) + N.z p.z  with p = x_v;  the ten terms are
 *       N.x N.x, N.x N.y, N.x N.z, N.y N.y, N.y N.z, N.z N.z,   N.x d, N.y d, N.z d,   d d
 *   None of them depends on the orientation of (u, w).
 * Vertex quadric.  Q_v = (A00 A01 A02 A11 A12 A22, b0 b1 b2, c) starts at +0.0 and adds, term by term:  for u in ring(v) ascending, the
 *   terms of (v, u, omin(v,u)), then, if omax(v,u) != omin(v,u), those of (v, u, omax(v,u)).  On a manifold interior vertex every face is
 *   met twice, which scales every quadric alike.  No float atomic.
 * Candidates.  An edge (a, b), a < b, is a candidate when  count == 2,  a and b are not both fixed,  ring(a) and ring(b) have exactly two
 *   common vertices (the link condition),  and not  |ring(a)| == |ring(b)| == 3  (the tetrahedron, which would fold flat).  An edge with
 *   two faces and a free end that fails the last two is counted in rejected_link.
 * Target and cost.  Q = Q_a + Q_b component by component;  m = 0.5 (x_a + x_b).  If a is fixed x = x_a, else if b is fixed x = x_b, else
 *       lam = reg ((A00 + A11) + A22);  if not lam > 0:  x = m;  else
 *       d00 = A00 + lam; d11 = A11 + lam; d22 = A22 + lam;   r_j = b_j + lam m_j
 *       l10 = A01 / d00;  l20 = A02 / d00;  e1 = d11 - l10 A01;  t21 = A12 - l20 A01;  l21 = t21 / e1;  e2 = (d22 - l20 A02) - l21 t21
 *       z1 = r1 - l10 r0;  z2 = (r2 - l20 r0) - l21 z1;  x2 = z2 / e2;  x1 = z1 / e1 - l21 x2;  x0 = (r0 / d00 - l10 x1) - l20 x2
 *   and x = m if a component of that x is not finite.  With  Ax_0 = (A00 x0 + A01 x1) + A02 x2  and Ax_1, Ax_2 alike,
 *       cost = (((x0 Ax_0 + x1 Ax_1) + x2 Ax_2) - 2 ((b0 x0 + b1 x1) + b2 x2)) + c,   0 unless cost > 0.
 *   t = x rounded to fp32 is where the survivor goes.
 * No flips.  For every face and every corner v of it that is not fixed, with the other corners p, q:  for u in ring(v), u not p or q,
 *   (v, u) a candidate:  N = (P1 - P0) x (P2 - P0) over the face's corners in its own order, N' the same with corner v at t widened;
 *   the candidate is dropped unless  (N'.x N.x + N'.y N.y) + N'.z N.z > 0  (rejected_flip).  Validity is settled before the selection.
 * Independent set.  key = (the bits of cost rounded to fp32) << 32 | owner.  Every valid candidate takes the 64-bit minimum of its key
 *   on claim[v] for every v of ring(a) U ring(b) (which holds a and b); it is SELECTED iff it holds every one of them.  Two selected
 *   edges have disjoint closed neighbourhoods: no face is touched by two collapses and the link and flip tests stay true.  The cheapest
 *   valid candidate is always selected.  Ties between equal costs break by owner, the edge's lowest half-edge number: the result is NOT
 *   invariant under a permutation of the faces.
 * Budget.  need = F_b > target_faces ? (F_b - target_faces + 1) / 2 : 0.  The selected edges whose key has fewer than `need` selected
 *   keys of the image below it collapse (an all-pairs count staged in LDS, only when more than `need` are selected): the image ends at
 *   target_faces or one below, unless the candidates run out first.
 * Apply.  The survivor s is the fixed end if there is one, else a; unless fixed it moves to t (verts is updated IN PLACE).  The other
 *   end r gets parent[r] = s.  parent [n_verts] int32 holds batch-global vertex numbers, parent[i] == i before the first round.
 *   faces_out [n_faces][3] (the bound; the first sum of faces_out rows are used): every face with its corners i replaced by
 *   parent[i] that still has three distinct corners, in the input order (an integer block scan).
 * fixed_out [n_verts] bytes, or NULL: 1 for a vertex that is FIXED in this round's input.
 * counts [SC_MESH_DECIMATE_FIELDS][n_images] int64, row by row: 0 faces_out, 1 selected, 2 collapsed, 3 candidates (before the flip
 *   test), 4 rejected_link, 5 rejected_flip, 6 fixed_vertices.
 * Only integer atomics decide anything: the same bits from run to run, for any batch, stream and table_slots (the edge table of
 * sc_mesh_subdivide).  14 launches on `stream` (3 when n_faces == 0), no wait on another workgroup, no host synchronisation.  scratch:
 * sc_mesh_decimate_scratch_bytes(n_images, n_verts, n_faces, table_slots) bytes, 16-byte aligned, contents irrelevant on entry (0 for
 * sizes the entry point refuses).  n_images <= 0 returns 0; hipErrorInvalidValue for n_images > 65535, n_faces > 2^26, n_verts > 2^30,
 * a negative count or target, a reg that is not > 0, a bad table_slots, a NULL pointer or a misaligned scratch (verts and parent may be
 * NULL when n_verts == 0, faces and faces_out when n_faces == 0, fixed_out always).
 *
 * sc_mesh_decimate_compact, once after the last round: the vertices that a face still uses, in ascending input number -> verts_out,
 * fixed_out (the caller's `fixed` bytes of those vertices) and v_count_out [n_images]; faces_out [n_faces][3] renumbered;
 * vertex_map [n_verts]: the image-local output number of the vertex at the end of i's parent chain, -1 if that one is not used.  4
 * launches; `scratch` as above (the bytes of a round of the same sizes suffice).                                                         */
#define SC_MESH_DECIMATE_FIELDS 7
long long sc_mesh_decimate_scratch_bytes(int n_images, int n_verts, int n_faces, int table_slots);
int sc_mesh_decimate_round(float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images, int n_verts,
                           int n_faces, int table_slots, int target_faces, double reg, void* scratch, int32_t* parent, int32_t* faces_out,
                           uint8_t* fixed_out, int64_t* counts, int32_t* flags, void* stream);
int sc_mesh_decimate_compact(const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images, int n_verts,
                             int n_faces, const int32_t* parent, const uint8_t* fixed, void* scratch, float* verts_out, int32_t* faces_out,
                             int32_t* vertex_map, uint8_t* fixed_out, int64_t* v_count_out, void* stream);

/* ---- validity: pairs of faces of a mesh that properly cross (csrc/mesh_intersect.hip) -------------------------------------------------
 * What ops.mesh_self_intersections runs and {idx}_mesh_selfx.txt reports (`--mesh.self_intersect`).  A batch of packed meshes: verts
 * [n_verts][3] fp32, faces [n_faces][3] with image-local indices, v_count / f_count [n_images] int32 on the device, non-negative, summing
 * to n_verts / n_faces (the form of sc_point_mesh_distance above).  Everything below is per image; faces are numbered image-locally.
 * tests/mesh_intersect_ref.py restates every rule in numpy.  The file is built without contraction: every operation is rounded once.
 *
 * Sign of a point against a plane, sign3(a, b, c, d) in {-1, 0, +1}.  The fp32 coordinates are widened to float64, then
 *       ad = a - d;  bd = b - d;  cd = c - d                                   (per component)
 *       m1 = bd.x cd.y;  m2 = bd.y cd.x;  m3 = cd.x ad.y;  m4 = cd.y ad.x;  m5 = ad.x bd.y;  m6 = ad.y bd.x
 *       det  = (ad.z (m1 - m2) + bd.z (m3 - m4)) + cd.z (m5 - m6)
 *       perm = ((|m1| + |m2|) |ad.z| + (|m3| + |m4|) |bd.z|) + (|m5| + |m6|) |cd.z|
 *   sign3 = 0 if |det| <= 2^-49 perm, else the sign of det.  2^-49 = 16 eps covers Shewchuk's static bound for this expansion (about
 *   7 eps times the permanent) and the three roundings of differences that are not exact in float64: a NON-ZERO sign3 is the sign of the
 *   exact determinant of the fp32 coordinates.  That is the property the whole check rests on.
 * Segment against triangle.  pierces(p, q; a, b, c) holds when  sign3(a,b,c,p) sign3(a,b,c,q) == -1  and  sign3(p,q,a,b), sign3(p,q,b,c),
 *   sign3(p,q,c,a) are equal and not zero: the ends lie strictly on both sides of the plane and the segment passes strictly inside.
 * Edges.  The face (i0, i1, i2) has the edges (v0,v1), (v1,v2), (v2,v0), in this orientation; the edge OPPOSITE corner s is
 *   (v_{(s+1)%3}, v_{(s+2)%3}).  A triangle enters sign3 and pierces in its own corner order.
 * A pair of faces, A the lower-numbered and B the higher, by the vertex indices they share:
 *       two or three:  never a hit (neighbours across an edge, duplicates) and not a pair at all;
 *       one, corner sa of A and sb of B:  a hit iff A's edge opposite sa pierces B or B's edge opposite sb pierces A;
 *       none:  a hit iff one of A's three edges pierces B or one of B's three edges pierces A.
 *   A face that repeats an index takes no part in any pair and is counted as degenerate.  Early exits are taken where signs settle the
 *   outcome (all of A strictly on one side of B's plane); the result is the plain definition's.
 * The rule is STRICT: it counts proper crossings only.  Contacts with a zero sign -- a vertex on a face, an edge through an edge,
 *   coplanar overlap, a crossing too close to call at 2^-49 -- are not hits.  Every counted pair truly intersects; the count is a lower
 *   bound on the pairs that touch.
 * counts [3][n_images] int64, row by row: 0 pairs = the hits, 1 pairs_vertex = those that share one vertex, 2 box_pairs = the unordered
 *   pairs of faces that take part, share at most one index and whose closed fp32 bounding boxes overlap (raw coordinates, no slack): a
 *   function of the mesh alone, there so that a broad phase that drops or repeats a pair shows.  A hit implies such an overlap.
 * face_counts [2][n_images] int32: 0 faces_hit = faces in at least one hit, 1 degenerate = faces in range that repeat an index.
 * hits [n_faces] int32: per packed face, the hits it is part of (their sum is 2 pairs).  partner [n_faces] int32: the lowest face it
 *   crosses, -1 without one.
 * flags [2] int32: 0 is set to 1 when a vertex of the batch has a component that is not finite or of magnitude >= 1e15, 1 when a face
 *   has an index outside [0, v_count[b]); such a face is never dereferenced and takes no part.  The caller raises for both; the other
 *   outputs are then unspecified.
 * brute != 0: all pairs, a thread per face, 256 higher-numbered faces at a time staged in LDS.  brute == 0: the triangle grid of
 *   sc_point_mesh_distance (csrc/triangle_grid.hpp); a pair whose boxes overlap is tested once, by the thread of its lower-numbered face
 *   in the cell that holds the component-wise maximum of the two box minima; a face on its image's large list is walked by a wave against
 *   every higher-numbered face of its image, and every other face also walks the higher-numbered faces of that list; an image whose grid
 *   is invalid (zero extent) takes the all-pairs path.  Both give the same integers in every output.
 * Integer atomics only (add on hits and the counters, min on partner): the same bits from run to run, for any batch, stream and face
 *   order; the integers permute with the faces.  One stream, no wait on another workgroup, no host synchronisation.  scratch:
 * sc_mesh_self_intersections_scratch_bytes(n_images, n_verts, n_faces) bytes of device memory, 16-byte aligned, contents irrelevant on
 * entry (-1 for sizes the entry point refuses).  n_images <= 0 returns 0 and launches nothing; hipErrorInvalidValue for n_images > 65535,
 * n_faces > 2^26, a negative count, a NULL pointer or a misaligned scratch (verts may be NULL when n_verts == 0; faces, hits and partner
 * when n_faces == 0).                                                                                                                     */
long long sc_mesh_self_intersections_scratch_bytes(int n_images, int n_verts, int n_faces);
int sc_mesh_self_intersections(const float* verts, const int32_t* faces, const int32_t* v_count, const int32_t* f_count, int n_images,
                               int n_verts, int n_faces, int brute, void* scratch, long long* counts, int32_t* face_counts, int32_t* hits,
                               int32_t* partner, int32_t* flags, void* stream);

/* ---- camera algebra of a render -------------------------------------------------------------------
 * sc_camera_rays_*: utils/camera.py:157-196 (get_center_and_ray on the rendered pixels only) + the normalisation of
 * model/renderer.py:69-76.  pose [n_images][3][4] = [R|t] world->camera, intr [n_images][3][3], ray_idx
 * [n_images][rays_per_image] int64 pixel indices (y*W + x) or NULL (= all pixels 0..rays_per_image-1).  Outputs per
 * ray: cam_loc [.][3] (camera centre, repeated), ray_dirs [.][3] (unit), depth_fac [.] (= |dir| / |unnormalised ray|).
 * Perspective model.  The backward returns d/d pose and d/d intr (g_* inputs may be NULL = zero).                */
int sc_camera_rays_forward(const float* pose, const float* intr, const long long* ray_idx, int n_images,
                           int rays_per_image, int image_width, float* cam_loc, float* ray_dirs, float* depth_fac,
                           void* stream);
int sc_camera_rays_backward(const float* pose, const float* intr, const long long* ray_idx, int n_images,
                            int rays_per_image, int image_width, const float* g_cam_loc, const float* g_ray_dirs,
                            const float* g_depth_fac, float* g_pose, float* g_intr, void* stream);

/* sc_pose_from_trig_*: model/graph.py:272-293 (pred_pose) with utils/camera.py:105-155,198-211: (cos,sin) of azimuth,
 * elevation, roll [n_images][2], scale_focal, scale_dist [n_images] -> pose [n_images][3][4] = [Rz Rx Ry P | (0,0,
 * cam_dist*scale_dist)], intr [n_images][3][3] = [[f W,0,W/2],[0,f H,H/2],[0,0,1]], f = focal*scale_focal.        */
int sc_pose_from_trig_forward(const float* azim, const float* elev, const float* theta, const float* scale_focal,
                              const float* scale_dist, int n_images, float cam_dist, float focal, int image_width,
                              int image_height, float* pose, float* intr, void* stream);
int sc_pose_from_trig_backward(const float* azim, const float* elev, const float* theta, const float* scale_focal,
                               const float* scale_dist, int n_images, float cam_dist, float focal, int image_width,
                               int image_height, const float* g_pose, const float* g_intr, float* g_azim,
                               float* g_elev, float* g_theta, float* g_scale_focal, float* g_scale_dist, void* stream);

/* ---- the [n_images]-sized arithmetic around the view estimator (csrc/camera_prior.hip): one launch each way where the
 * reference spends dozens of [B]-shaped torch operators.
 * sc_estimator_head_*: model/view_estimator.py:62-75.  trig [n_rows][6] (extr_fc output), size_lin / persp_lin [n_rows]
 *   (size_fc / perspect_fc outputs) -> azim, elev, theta [n_rows][2] = F.normalize of the three pairs (eps 1e-12),
 *   scale_focal = 1 + tanh(persp_lin) * persp_range, scale_dist = (1 + tanh(size_lin) * size_range) * scale_focal.
 *   Backward: the rows are n_groups stacked image sets of n_rows / n_groups rows (<= 8 groups); grads is a HOST array of
 *   5 * n_groups device pointers (group-major: azim, elev, theta, scale_focal, scale_dist of that group, each
 *   [rows][2] or [rows]; NULL = that output was not differentiated).  Returns -1 for a bad group count.            */
int sc_estimator_head_forward(const float* trig, const float* size_lin, const float* persp_lin, int n_rows,
                              float size_range, float persp_range, float* azim, float* elev, float* theta,
                              float* scale_focal, float* scale_dist, void* stream);
int sc_estimator_head_backward(const float* trig, const float* size_lin, const float* persp_lin, int n_rows,
                               float size_range, float persp_range, const float* const* grads, int n_groups,
                               float* g_trig, float* g_size_lin, float* g_persp_lin, void* stream);

/* sc_camera_prior_*: model/loss.py:99-167 -- cam_margin_loss (elevation and roll ranges in degrees, eps = margin_eps),
 *   cam_uniform_loss (sorted (cos, sin, cos*sin) of the azimuth against the sorted uniform grid; emd_p 1 or 2) and
 *   cam_sym_loss against the estimator's outputs on the mirrored images (flip_*), all [n_images][2].
 *   out [3] = (cam_margin, cam_uniform, cam_sym); grads [6][n_images][2] = d margin/d elev, d margin/d theta,
 *   d uniform/d azim, d sym/d azim, d sym/d elev, d sym/d theta.  One workgroup; n_images <= sc_camera_prior_max_images()
 *   (1024), otherwise -1.  The backward scales by the upstream gradients of the three values (device scalars, NULL = 0)
 *   and also returns d sym/d flip_*.                                                                               */
int sc_camera_prior_max_images(void);
int sc_camera_prior_forward(const float* azim, const float* elev, const float* theta, const float* flip_azim,
                            const float* flip_elev, const float* flip_theta, int n_images, float elev_lo, float elev_hi,
                            float theta_lo, float theta_hi, float margin_eps, int emd_p, float* out, float* grads,
                            void* stream);
int sc_camera_prior_backward(const float* grads, int n_images, const float* G_margin, const float* G_uniform,
                             const float* G_sym, float* g_azim, float* g_elev, float* g_theta, float* g_flip_azim,
                             float* g_flip_elev, float* g_flip_theta, void* stream);

/* sc_transform_normal_*: utils/camera.py:98-103 -- out[b][r][:] = normals[b][r][:] @ R_b with R_b the rotation block of
 *   pose [n_images][3][4].  Backward: g_pose [n_images][3][4] (translation column zero); the normals are data.      */
int sc_transform_normal_forward(const float* normals, const float* pose, int n_images, int n_per_image, float* out,
                                void* stream);
int sc_transform_normal_backward(const float* normals, const float* g_out, int n_images, int n_per_image, float* g_pose,
                                 void* stream);

/* sc_loss_total_*: model/runner.py:294-305 -- total = sum_k weights[k] * *values[k] added in index order (<= 16 terms;
 *   values is a HOST array of device scalars, weights a HOST array), bad = 1 if any term is NaN/Inf.  Backward:
 *   g_values[k] = weights[k] * *G.                                                                                 */
int sc_loss_total_forward(const float* const* values, const float* weights, int n_terms, float* total, unsigned char* bad,
                          void* stream);
int sc_loss_total_backward(const float* weights, int n_terms, const float* G, float* g_values, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 3x3 / stride 1 / pad 1 convolution of the ResNet-18/34 trunks (torchvision BasicBlock conv1/conv2 behind
 * model/graph.py:50-54 and model/view_estimator.py:40-42), NCHW fp32, on the fp32 matrix pipe (csrc/conv3x3.hip).
 * hw = side of the square feature map: 56, 28, 14 or 7 (anything else returns -1: the caller keeps MIOpen for it).
 *   sc_conv3x3_pack_floats  size of the kernel-ready weight image (floats), -1 for an unsupported shape
 *   sc_conv3x3_pack         w [cout][cin][3][3] -> w_pack.  transpose_flip = 1 writes the filter of the backward-data pass,
 *                           w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx], for w stored [cin][cout][3][3] in THIS call's naming
 *                           (cin = channels of dL/dy, cout = channels of dL/dx)
 *   sc_conv3x3_forward      out [batch][cout][hw][hw] = conv(x [batch][cin][hw][hw], w), fully overwritten.
 *                           dL/dx = sc_conv3x3_forward(dL/dy, pack(w, transpose_flip = 1)).
 *                           workspace: sc_conv3x3_workspace_floats(hw) floats of device scratch (partial tiles of the
 *                           workgroups that share the last round's tiles; summed in a fixed order by a second launch).
 *   sc_conv3x3_pack_multi   the same images for MANY filters in one launch (a network's filters change once per optimizer
 *                           step): table = n <= 128 rows of 6 int64 on the device, {address of w, first float of the image inside dst,
 *                           cin, cout, sc_conv3x3_tile_channels(hw), transpose_flip}, rows sorted by first float; total = floats
 *                           of all images.  Image e is then  dst + row[1]  and has sc_conv3x3_pack_floats(cin, cout, hw) floats.  */
long long sc_conv3x3_pack_floats(int cin, int cout, int hw);
long long sc_conv3x3_workspace_floats(int hw);
int sc_conv3x3_tile_channels(int hw);
int sc_conv3x3_pack_multi(const long long* table, int n, float* dst, long long total, void* stream);
/* The same table, for the case that EVERY row is a split image (transpose_flip bit 1) with 64-channel tiles (sc_conv3x3_tile_channels_split
 * = 64): one workgroup per 64 x 16 x 9 unit of a filter (a pair of K-steps: nine tap-pair images, see csrc/conv3x3.hip), contiguous reads
 * and writes (byte-identical images); total % 13824 must be 0.                                                                          */
int sc_conv3x3_pack_multi_units(const long long* table, int n, float* dst, long long total, void* stream);
int sc_conv3x3_pack(const float* w, float* w_pack, int cin, int cout, int hw, int transpose_flip, void* stream);
int sc_conv3x3_forward(const float* x, const float* w_pack, float* out, float* workspace, int batch, int cin, int cout, int hw,
                       void* stream);

/* The same convolution with fp32-ACCURATE products on the bf16 matrix pipe (opt-in, `--hip.conv3x3_split`): every operand is split
 * exactly into three bf16 pieces (x = p0 + p1 + p2), the six products a_p b_q with p + q <= 2 are accumulated in fp32 (what is dropped
 * is < 2^-23 |a||b| per product); 6 bf16 MFMAs replace 16 fp32-MFMA passes.  Same tensors and semantics as sc_conv3x3_forward; the
 * filter image is written by sc_conv3x3_pack with bit 1 of transpose_flip set (or flags | 2 in a sc_conv3x3_pack_multi row) and has
 * sc_conv3x3_pack_floats_split floats; tile width / workspace: the _split queries.                                                   */
long long sc_conv3x3_pack_floats_split(int cin, int cout, int hw);
long long sc_conv3x3_workspace_floats_split(int hw);
int sc_conv3x3_tile_channels_split(int hw);
int sc_conv3x3_forward_split(const float* x, const float* w_pack, float* out, float* workspace, int batch, int cin, int cout, int hw,
                             void* stream);
/* out = conv(x, w) + addend, the sum formed in the store epilogue (addend: a tensor of the output's shape; split != 0: w_pack is a split image).
 * Used for d L / d x of a residual block: backward-data of conv1 + the gradient of the skip branch (model/graph.py's torchvision BasicBlock:
 * autograd's accumulation of the two uses of the block input).                                                                      */
int sc_conv3x3_forward_add(const float* x, const float* w_pack, const float* addend, float* out, float* workspace, int batch, int cin,
                           int cout, int hw, int split, void* stream);

/* 3x3 / stride 2 / pad 1 (BasicBlock.conv1 of layer2-4; torchvision layer{2,3,4}.0.conv1 behind model/graph.py:50-54 and
 * model/view_estimator.py:40-42), same kernel family: hw = side of the INPUT map (56, 28 or 14), out [batch][cout][hw/2][hw/2].
 * Forward filter image: sc_conv3x3_pack with bit 2 (value 4) of transpose_flip set, sc_conv3x3s2_pack_floats floats.
 * Backward-data (sc_conv3x3s2_backward_data: gx [batch][cin][hw][hw] from gy [batch][cout][hw/2][hw/2]): four stride-1 sub-convolutions
 *   over the gradient map, one per output parity, each with the 1 / 2 / 2 / 4 filter taps that reach it -- every product of the transposed
 *   convolution once; exact three-piece bf16 operand splits with fp32 accumulation (the arithmetic of sc_conv3x3_forward_split).  Filter
 *   image: sc_conv3x3s2_bd_pack from the FORWARD filter w [cout][cin][3][3], sc_conv3x3s2_bd_pack_floats floats; workspace
 *   sc_conv3x3s2_bd_workspace_floats(hw) floats.  cout % 8 == 0.
 * Backward-weight (sc_conv3x3s2_wgrad: dw [cout][cin][3][3] from gy and x [batch][cin][hw][hw]): csrc/conv3x3_wgrad.hip with stride-2 patch
 *   addressing, fp32 MFMA, fixed summation order; workspace sc_conv3x3_wgrad_workspace_floats(cin, cout) floats; cin, cout % 64 == 0. */
long long sc_conv3x3s2_bd_pack_floats(int cin, int cout, int hw);
long long sc_conv3x3s2_bd_workspace_floats(int hw);
int sc_conv3x3s2_bd_pack(const float* w, float* w_pack, int cin, int cout, int hw, void* stream);
int sc_conv3x3s2_backward_data(const float* gy, const float* w_pack, float* gx, float* workspace, int batch, int cin, int cout, int hw,
                               void* stream);
int sc_conv3x3s2_wgrad(const float* gy, const float* x, float* dw, float* workspace, int batch, int cin, int cout, int hw, void* stream);
long long sc_conv3x3s2_pack_floats(int cin, int cout, int hw);
long long sc_conv3x3s2_workspace_floats(int hw);
int sc_conv3x3s2_forward(const float* x, const float* w_pack, float* out, float* workspace, int batch, int cin, int cout, int hw,
                         void* stream);

/* Weight gradient of the same convolution (csrc/conv3x3_wgrad.hip):  dw [cout][cin][3][3] = sum over the batch of gy (x) shifted x,
 * gy [batch][cout][hw][hw], x [batch][cin][hw][hw], fully overwritten, fixed summation order.  cin and cout must be multiples of 64
 * (otherwise hipErrorInvalidValue; sc_conv3x3_wgrad_workspace_floats returns -1): the caller keeps MIOpen for other shapes.
 * workspace: sc_conv3x3_wgrad_workspace_floats(cin, cout) floats (one partial 64 x 64 x 9 block per workgroup).                       */
long long sc_conv3x3_wgrad_workspace_floats(int cin, int cout);
int sc_conv3x3_wgrad(const float* gy, const float* x, float* dw, float* workspace, int batch, int cin, int cout, int hw, void* stream);
/* The same gradient with fp32-accurate products on the bf16 matrix pipe (the arithmetic of sc_conv3x3_forward_split: exact three-way
 * bf16 split of BOTH operands, the six piece products with p + q <= 2, smallest first, fp32 accumulate); same arguments and workspace. */
int sc_conv3x3_wgrad_split(const float* gy, const float* x, float* dw, float* workspace, int batch, int cin, int cout, int hw, void* stream);

/* The stem of the trunks (torchvision ResNet.conv1: 7x7 / stride 2 / pad 3, 3 -> 64 channels, 224 x 224 inputs only; csrc/conv_stem.hip):
 *   sc_conv_stem_forward   out [batch][64][112][112] = conv(x [batch][3][224][224], w [64][3][7][7]), fully overwritten
 *   sc_conv_stem_wgrad     dw [64][3][7][7] = weight gradient from gy [batch][64][112][112] and x, fixed summation order;
 *                          workspace: sc_conv_stem_wgrad_workspace_floats() floats.  (The input is data: no backward-data.)          */
long long sc_conv_stem_wgrad_workspace_floats(void);
int sc_conv_stem_forward(const float* x, const float* w, float* out, int batch, void* stream);
int sc_conv_stem_wgrad(const float* gy, const float* x, float* dw, float* workspace, int batch, void* stream);

/* The 1x1 / stride 2 shortcut convolutions of the trunks (torchvision BasicBlock.downsample[0]; csrc/conv1x1s2.hip), NCHW fp32,
 * hin = side of the (square, even) input map, cin and cout multiples of 64 (otherwise hipErrorInvalidValue / -1):
 *   sc_conv1x1s2_forward        out [batch][cout][hin/2][hin/2] = sum_ci w[cout][cin] x[batch][cin][2y][2x]
 *   sc_conv1x1s2_backward_data  gx [batch][cin][hin][hin] from gy [batch][cout][hin/2][hin/2]: fully written (zeros at odd positions)
 *   sc_conv1x1s2_wgrad          dw [cout][cin] from gy and x, fixed summation order; workspace: the _workspace_floats query.        */
long long sc_conv1x1s2_wgrad_workspace_floats(int cin, int cout);
int sc_conv1x1s2_forward(const float* x, const float* w, float* out, int batch, int cin, int cout, int hin, void* stream);
int sc_conv1x1s2_backward_data(const float* gy, const float* w, float* gx, int batch, int cin, int cout, int hin, void* stream);
int sc_conv1x1s2_wgrad(const float* gy, const float* x, float* dw, float* workspace, int batch, int cin, int cout, int hin, void* stream);

/* ---- one call per BasicBlock (csrc/block.hip) ------------------------------------------------------------------------------------------
 * torchvision BasicBlock with stride 1 and no shortcut convolution, as the reference's ResNet-18 / 34 trunks run it (model/graph.py:50-54,
 * model/view_estimator.py:40-42):   out = relu( bn2( conv2( relu( bn1( conv1(x) ) ) ) ) + x ),   x, y1, a1, y2, out: [batch][channels][hw][hw].
 * Host glue over the entry points above (same launches, same order, same results): the caller fills one argument block per call.
 *   forward : reads x, pf1, pf2 (filter images of sc_conv3x3_pack, forward orientation), the BatchNorm parameters / running statistics
 *             (rm / rv / nt may be NULL); writes y1 = conv1(x), a1 = relu(bn1(y1)), y2 = conv2(a1), out, st1, st2 ([2][groups][channels]:
 *             save_mean | save_rstd).
 *   backward: reads d_out and what the forward wrote, pb1 / pb2 (backward-data filter images); writes dy2, da1, dy1 (scratch the caller
 *             provides), dgb1 / dgb2 ([2][channels]: dgamma | dbeta), gw1 / gw2 ([channels][channels][3][3], NULL: skipped) and -- when
 *             need_dx -- dres (scratch) and dx = dL/dx (both uses of x summed).
 * Workspaces: conv_ws sc_conv3x3_workspace_floats[_split](hw), bn_ws 2 * (2048 + channels * groups), wgrad_ws
 * sc_conv3x3_wgrad_workspace_floats(channels, channels) floats.  split != 0: the bf16x3-split arithmetic of sc_conv3x3_forward_split /
 * sc_conv3x3_wgrad_split.  Returns the first non-zero status of the calls it makes.                                                       */
typedef struct sc_block_args {
    const float *x, *pf1, *pf2, *pb1, *pb2;
    const float *g1, *b1, *g2, *b2;
    float *rm1, *rv1, *rm2, *rv2;
    int64_t *nt1, *nt2;
    float *y1, *a1, *y2, *out, *st1, *st2;
    float *conv_ws, *bn_ws, *wgrad_ws;
    const float* d_out;
    float *dy2, *dres, *da1, *dy1, *dx, *gw1, *gw2, *dgb1, *dgb2;
    int batch, channels, hw, groups, training, split, need_dx;
    float mom1, eps1, mom2, eps2;
} sc_block_args;
int sc_basic_block_forward(const sc_block_args* args, void* stream);
int sc_basic_block_backward(const sc_block_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 1x1 "Bottleneck_Linear" blocks (csrc/bottleneck.hip): a linear layer WITHOUT bias on row vectors followed by BatchNorm over the rows,
 * optional residual and ReLU, one launch per linear each way.  Replaces, per block, the reference's two nn.Conv2d(C, C, 1) + two
 * nn.BatchNorm2d on 1x1 maps (model/view_estimator.py:6-33 heads, model/graph.py:16-44 latent projectors): rocBLAS products + separate
 * BatchNorm launches before.  x [N][Cin], w [Cout][Cin] (torch layout), y / out / res [N][Cout]; `groups` stacked sub-batches of N / groups
 * rows with their own statistics (save_mean / save_rstd [groups][Cout]); running statistics (may be NULL when training) are updated
 * once per group in order, *n_tracked += groups.  Limits: N <= 128, groups <= 4, Cin % 64 == 0, Cout % 16 == 0
 * (sc_linear_bn_supported says whether a shape is taken).  Fixed summation orders: bit-reproducible.
 * The reduction length of each of the three products is split over four waves in steps of 16, so it must be a multiple of 64: Cin in the
 * forward pass (above); Cnext in sc_linear_bn_backward when g_out is NULL; Cout in sc_linear_backward_data (whose Cin, the columns of
 * dx, need only Cin % 16 == 0, and N <= 128).  Anything else is refused with hipErrorInvalidValue before a launch.
 *   forward:   y = x w^T;  out = [relu]( gamma (y - mean) rstd + beta [+ res] )
 *   backward:  g = (g_out, or gy_next [N][Cnext] x w_next [Cnext][Cout] when g_out is NULL) [+ g_add]; ReLU mask from `out`;
 *              g_res (may be NULL) receives the masked gradient (= gradient of `res`); BatchNorm backward -> gy [N][Cout];
 *              dw [Cout][Cin] = gy^T x; dgamma, dbeta [Cout]
 *   data:      dx [N][Cin] = gy [N][Cout] w [Cout][Cin] [+ g_add]                                                                  */
int sc_linear_bn_supported(int N, int Cin, int Cout, int groups);
int sc_linear_bn_forward(const float* x, const float* w, const float* gamma, const float* beta, const float* res, float* y, float* out,
                         float* save_mean, float* save_rstd, float* run_mean, float* run_var, int64_t* n_tracked, int N, int Cin,
                         int Cout, int groups, int training, int relu, float eps, float momentum, void* stream);
int sc_linear_bn_backward(const float* g_out, const float* gy_next, const float* w_next, const float* g_add, int Cnext, const float* out,
                          const float* y, const float* save_mean, const float* save_rstd, const float* gamma, const float* x, float* gy,
                          float* g_res, float* dw, float* dgamma, float* dbeta, int N, int Cin, int Cout, int groups, int training, int relu,
                          void* stream);
int sc_linear_backward_data(const float* gy, const float* w, const float* g_add, float* dx, int N, int Cin, int Cout, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-image biases of the conditioned MLP layers (csrc/latent_bias.hip): the latent columns of a layer act on the [B][Z] latent once per
 * image -- the reference repeats the latent per sample point (model/implicit.py:166, model/renderer.py:89).
 *   out [B][NL][64] = bias [NL][64] + (l < L ? post[l] : 0) * z [B][Z] lat[l * 64 + ch][Z]^T      (post may be NULL = 1)
 *   backward: g [B][NL][64] -> g_z [B][Z] (may be NULL), g_lat [L * 64][Z], g_bias [NL][64].  Every element is one fixed-order sum:
 *   results do not depend on the batch size.                                                                                          */
int sc_latent_bias_forward(const float* z, const float* lat, const float* bias, const float* post, float* out, int B, int Z, int L, int NL,
                           void* stream);
int sc_latent_bias_backward(const float* g, const float* z, const float* lat, const float* post, float* g_z, float* g_lat, float* g_bias,
                            int B, int Z, int L, int NL, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Silhouette ray choice of the Pix3D training loader (csrc/silhouette_rays.hip; reference data/pix3d.py:230-239 ->
 * utils/util.py:237-248).  One workgroup per mask; 1 <= H, W <= 512, otherwise hipErrorInvalidValue.
 *   sc_silhouette_distance: masks [n][H][W] fp32 (inside: > 0.5) -> dist [n][H][W] fp32 = Euclidean distance from the pixel
 *     centre to the nearest pixel centre of the other class minus 0.5 (the image border is no boundary), bit-identical to
 *     float32(sqrt(float64(dx^2 + dy^2)) - 0.5).  A mask of one class only: dist = 0 everywhere.
 *   sc_silhouette_rays: dist [n][H][W], seeds [n] int64 -> ray_idx [n][n_rays] int64, 1 <= n_rays <= H*W (else
 *     hipErrorInvalidValue): the n_rays smallest keys -log(u_i) * (double(dist_i) + uniform_fac) in increasing order, ties to
 *     the lower index -- a draw without replacement with weights 1 / (dist + uniform_fac) in successive-sampling order.  u_i is
 *     a splitmix64 hash of (seed, i) in (0, 1] (formula in the source), so a mask's draw depends on its own seed only.            */
int sc_silhouette_distance(const float* masks, int n, int H, int W, float* dist, void* stream);
int sc_silhouette_rays(const float* dist, int n, int H, int W, int n_rays, double uniform_fac, const long long* seeds,
                       long long* ray_idx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CLIP preprocessing of Pix3D loader images (csrc/clip_preprocess.hip; reference data/pix3d.py:278-289 in CLIP-annotation mode, then
 * openai/CLIP's _transform(n_px)).  rgba [n][H][W][4] uint8 (the loader's resized RGBA) -> out [n][3][n_px][n_px] fp32:
 *   q = alpha >= 128 ? c : bg (bg = -1: no composite, q = c); Pillow's 8-bit bicubic resize, horizontal pass then vertical pass,
 *   each output value clip8((2^21 + sum q * k) >> 22) with the int32 tables of data/clip_preprocess.py; (v / 255 - mean) / std.
 * Tables, centre crop included: h_bounds [n_px][2] (first source column, tap count), h_coef [n_px][h_taps]; v_bounds [n_px][2]
 * (first source row, tap count), v_coef [n_px][v_taps].  tmp: workspace of n * H * n_px * 4 bytes.  rgba, tmp and out 4-byte
 * aligned.  hipErrorInvalidValue for 1 > H, W > 16384, 1 > n_px > 2048, bg outside [-1, 255], taps outside [1, 1024],
 * n outside [0, 65535] or a NULL pointer; n = 0 launches nothing.                                                            */
int sc_clip_preprocess(const unsigned char* rgba, int n, int H, int W, int n_px, int bg, const int* h_bounds, const int* h_coef,
                       int h_taps, const int* v_bounds, const int* v_coef, int v_taps, unsigned char* tmp, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Turn-table GIF frames (csrc/vis_frames.hip; reference model/runner.py:417-424 -> utils/util_vis.py:35-44,68-80).  x: per-ray outputs
 * of the render chain, n_pixels rows of `channels` fp32 (the ray order of an image is row-major pixel order) -> out [n_pixels][3]
 * uint8 in one launch, the bytes the reference hands to PIL:
 *   kind 0 (RGB, channels 3):    trunc(clamp((x - lo) * scale, 0, 1) * 255)
 *   kind 1 (mask, channels 1):   i = trunc(clamp((x - lo) * scale, 0, 1) * 256), 256 -> 255, on all three channels (matplotlib's
 *                                `gray` colormap as get_heatmap applies it; its float64 -> fp32 -> * 255 round trip gives i back)
 *   kind 2 (normal, channels 3): x * 0.5 + 0.5 first (no contraction), then as kind 0
 * scale = fp32 1 / (hi - lo).  NaN writes 0.  hipErrorInvalidValue for n_pixels outside [0, 2^40], another kind / channels pair, a NULL
 * pointer or an out that is not 4-byte aligned; n_pixels = 0 launches nothing.                                                     */
int sc_vis_frames(const float* x, long long n_pixels, int channels, int kind, float lo, float scale, unsigned char* out, void* stream);

/* Coloured meshes (csrc/rgb_points.hip): RGBNetwork.forward (model/implicit.py:220-239) at arbitrary points, e.g. mesh vertices.
 * points [n_points][3]; grad [n_points][3] and feat (TBL64, ceil(n_points / 16) tiles) are what sc_sdf_forward / sc_sdf_forward_stream
 * wrote for those points; v_pack / dbias [n_images][3][64] as sc_rgb_composite_forward.  The image of point i is
 * min(16 * floor(i / 16) / n_per_image, n_images - 1), as in the SDF kernels; n_per_image must be a positive multiple of 16.
 * -> rgb [n_points][3] (sigmoid colours; bit-identical to the rgb_flat rows of sc_rgb_composite_forward_split at the same inputs: the
 *    same pre-split bf16x3 chain) and normal [n_points][3] = grad / max(|grad|, 1e-12).  Either output may be NULL (rgb NULL: feat,
 *    v_pack and dbias are not read; normal NULL: grad is not read).  Nothing is read or written past n_points.  n_points = 0 launches
 *    nothing; a negative n_points, n_per_image <= 0, n_per_image % 16 != 0 or n_images <= 0 returns hipErrorInvalidValue.             */
int sc_rgb_points_forward_split(const float* points, const float* grad, const float* feat, const float* v_pack,
                                const float* dbias, int n_points, int n_per_image, int n_images, int symmetric,
                                float* rgb, float* normal, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Largest connected component of the solid of a level grid (csrc/level_components.hip): the stage between the level grid and the
 * sc_marching_cubes_* / sc_isosurface_* entry points, for dropping detached "floaters".  level [n_images][S][S][S] fp32, S = n_axis.
 *   inside:      a voxel is inside iff level < iso, the corner predicate of the meshers (NaN and +Inf are outside, -Inf is inside).
 *   components:  of the inside voxels of ONE image under 6-connectivity (two voxels are joined iff they share a face; an edge or a
 *                corner is not enough); never across images.
 *   label:       the smallest linear index (x * S + y) * S + z of the component's voxels;  size: its voxel count.
 *   kept:        the component of the largest size; among components of equal size the one with the smallest label.
 *   level_out [n_images][S][S][S]: the bits of level everywhere (NaN payloads included), except at the inside voxels of components
 *                that are not kept, which hold iso + (iso - level) -- the value reflected to the outside, one fp32 subtraction and one
 *                fp32 addition (an exact sign flip for iso = 0).  level_out may be level itself.
 *   n_components, inside_voxels, kept_voxels [n_images] int32: components, inside voxels and voxels of the kept component of each
 *                image (0, 0, 0 without an inside voxel).  An image with no or one component comes back bit-identical.
 * Integer atomics only: the same bits from run to run, whatever n_images, the stream or sc_set_reserved_cus.  Five launches on `stream`,
 * no host synchronisation.  scratch: sc_level_largest_component_scratch_bytes(n_images, n_axis) bytes of device memory, 16-byte
 * aligned, contents irrelevant on entry (the query gives 0 for sizes the entry point refuses).  n_images <= 0 returns 0 and launches
 * nothing; hipErrorInvalidValue for n_images > 65535, n_axis outside [2, 1024], a NULL pointer or a misaligned scratch.            */
long long sc_level_largest_component_scratch_bytes(int n_images, int n_axis);
int sc_level_largest_component(const float* level, int n_images, int n_axis, float iso, float* level_out, int32_t* n_components,
                               int32_t* inside_voxels, int32_t* kept_voxels, void* scratch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Surface render (csrc/surface_hit.hip): the per-ray root finder between a value-only SDF pass over the S uniform samples of every ray
 * and the colour / normal evaluation at the surface point (Renderer.render_surface, `--hip.surface_render`).  All arithmetic is fp32,
 * every operation rounded once (no contraction), every comparison a true comparison (false when an operand is NaN).
 *
 * sc_ray_first_crossing: z_vals [n_rays][S], sdf [n_rays * S] (sample i of ray r at r * S + i), S = n_samples with
 * SC_N_SAMPLES_SUPPORTED, f_i = sdf_i - iso.  Per ray r:
 *   hit = 2  if f_0 <= 0 (the near end of the ray is already inside):  t_lo = t_hi = z_0, f_lo = f_hi = f_0;
 *   hit = 1  otherwise, at the SMALLEST i in [0, S - 2] with f_i > 0 and f_{i+1} <= 0 (outside -> inside; a NaN on either side never
 *            forms a bracket, inside -> outside pairs are passed over, a pair that lies across two 64-sample chunks counts like any
 *            other):  t_lo = z_i, f_lo = f_i, t_hi = z_{i+1}, f_hi = f_{i+1};
 *   hit = 0  otherwise:  t_lo = t_hi = z_0, f_lo = f_hi = f_0 (a NaN f_0 is written as it is; t stays finite).
 * Outputs t_lo, t_hi, f_lo, f_hi [n_rays] fp32 and hit [n_rays] int32, every element overwritten.  One 64-lane wave per ray, one
 * ballot per chunk of 64 samples, one pass over the ray, no atomics.
 *
 * sc_ray_bracket_step: one lane per ray; the bracket arrays are read and updated in place.  cam_loc, ray_dirs [n_rays][3] as
 * sc_camera_rays_forward writes them.
 *   update (only when f_new != NULL and hit == 1), with f = f_new[r] - iso the value at the previous query t_prev[r]:
 *            f > 0:  t_lo = t_prev, f_lo = f;      f <= 0:  t_hi = t_prev, f_hi = f;      f NaN: nothing changes.
 *   query, hit == 1:  d = f_lo - f_hi;  w = f_lo / d;  if !(d <= FLT_MAX) or !(w >= 0 && w <= 1) then w = 0.5 (d overflowed to Inf
 *            or a value is NaN: bisect);  x = t_lo + w * (t_hi - t_lo);  if !(x >= t_lo) then x = t_lo;  if !(x <= t_hi) then
 *            x = t_hi;  t = x.            hit != 1:  t = t_lo.
 *   t [n_rays] and points [n_rays][3] = cam_loc + t * ray_dirs (one multiplication, one addition: the ray sampler's expression) are
 *   overwritten for every ray, so a ray that misses still gets a finite point.  t_prev may be t itself; it is not read when f_new is
 *   NULL (and may then be NULL).
 * With f_lo > 0 >= f_hi on entry (what sc_ray_first_crossing leaves) the update keeps f_lo > 0 >= f_hi and t_lo <= t <= t_hi, and the
 * bracket never widens: regula falsi with a safeguard, K updates cost K value-only SDF evaluations of n_rays points.
 *
 * Plain vector stores, no atomics: the same bits run to run, whatever the batch or the stream.  n_rays <= 0 returns 0 and launches
 * nothing; hipErrorInvalidValue for an unsupported n_samples, n_rays > SC_SURFACE_HIT_MAX_RAYS or a NULL pointer (f_new / t_prev
 * excepted as above).                                                                                                          */
#define SC_SURFACE_HIT_MAX_RAYS (1 << 30)
int sc_ray_first_crossing(const float* z_vals, const float* sdf, int n_rays, int n_samples, float iso, float* t_lo, float* t_hi,
                          float* f_lo, float* f_hi, int32_t* hit, void* stream);
int sc_ray_bracket_step(const float* cam_loc, const float* ray_dirs, const float* f_new, const float* t_prev, int n_rays, float iso,
                        float* t_lo, float* t_hi, float* f_lo, float* f_hi, const int32_t* hit, float* t, float* points, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-triangle texture atlas (csrc/texture_bake.hip): the kernels between the indexed marching-cubes mesh and a textured OBJ
 * (eval_3D.mesh_texture, `--eval.texture`).  All arithmetic is fp32, every operation rounded once (no contraction), division correctly
 * rounded.  tests/texture_ref.py restates every line below in numpy.
 *
 * Layout, a pure function of the face index.  T = texels (4..32) is the side of a square cell; every cell holds two triangular charts.
 *   atlas:   A x A texels, A a power of two in 64..8192, n = A / T (integer division) cells per row and per column; one A serves every
 *            image of a call.  x runs to the right, y downward (image row 0 is y = 0).  Columns and rows >= n T belong to no cell.
 *   face f:  cell c = f >> 1, half h = f & 1;  the cell's origin is (X0, Y0) = (T (c % n), T (c / n)).
 *   texel (i, j) of a cell (i = x - X0, j = y - Y0, both in [0, T)) belongs to the lower half (h = 0) iff i + j <= T - 1, else to the upper.
 *   corners (cell-local texel indices, at texel centres):   lower p0 = (0, 0),     p1 = (T-3, 0), p2 = (0, T-3);
 *                                                           upper p0 = (T-1, T-1), p1 = (2, T-1), p2 = (T-1, 2)   (the lower chart
 *            rotated by 180 degrees: orientation is kept).
 *   barycentrics of texel (i, j):   lower  b1 = (float)i / (float)(T-3),        b2 = (float)j / (float)(T-3);
 *                                   upper  b1 = (float)(T-1-i) / (float)(T-3),  b2 = (float)(T-1-j) / (float)(T-3);
 *                                   b0 = (1 - b1) - b2.    Nothing is clamped: texels outside the triangle (the gutter) take the affine
 *            extrapolation in the triangle's plane, by at most (T-1)/(T-3) edge lengths from p0.  A bilinear footprint of a point inside
 *            the lower chart touches texels with i + j <= T-2 only, one inside the upper chart texels with i + j >= T only.
 *   OBJ texture coordinate of corner k of face f:  vt = ((X0 + pk.x + 0.5) / A, 1 - (Y0 + pk.y + 0.5) / A); both are exact in fp32, and
 *            so are u A - 0.5 and (1 - v) A - 0.5 there, so the look-up of a corner is that one texel.
 *
 * sc_texture_queries: one thread per texel (image b, row y < rows, column x < A); verts [n_verts][3] fp32 in grid-index units and faces
 * [n_faces][3] int32 (vertex numbers local to their image) as sc_marching_cubes_mesh_* write them; v_start, f_start, f_count [n_images]
 * int64 on the device: image b's faces are faces[f_start[b] .. f_start[b] + f_count[b]), its vertex k is verts[v_start[b] + k].
 *   used texel (x < n T, face f = 2 c + h < f_count[b]):  with v0, v1, v2 the face's vertices, per coordinate
 *            v = (b0 v0 + b1 v1) + b2 v2;    query = (float)lo + v * scale,    scale = (float)((hi - lo) / (double)(n_axis - 1))
 *            (lo, hi doubles: the positions the level grid was sampled at, eval_3D.mesh_attributes' expression);  face_of_texel = f.
 *   unused texel:  face_of_texel = -1;  query = that of texel (0, 0) of the image (corner p0 of its face 0: b0 = 1), or ((float)lo) x 3
 *            for an image without faces, so the networks see finite input.
 *   query [n_images][image_stride][3]: image b's texel (x, y) at row y A + x of its block; image_stride >= rows A, the rows behind
 *   rows A are not written (the caller's further queries of that image).  face_of_texel [n_images][rows A] int32.  A vertex number
 *   outside [0, n_verts) is read as vertex 0 or n_verts - 1 (no access outside verts); the caller keeps f_start + f_count <= n_faces.
 *
 * sc_texture_pack: rgb, normal [n_images][rows A][3] fp32 (the colours and unit normals at the queries) -> atlas, normal_atlas
 * [n_images][A][A][3] uint8, every byte written.  Used texel:  colour byte = trunc(clamp(c, 0, 1) * 255), normal byte =
 * trunc(clamp((n + 1) * 0.5, 0, 1) * 255); a NaN gives 0.  Texels with face_of_texel < 0 and rows >= `rows`: 127 on every channel.
 * One thread per four texels, 12-byte stores: both atlases 4-byte aligned.
 *
 * sc_texture_sample: the bilinear look-up a viewer performs.  atlas [n_images][A][A][C], fp32 (is_u8 = 0) or uint8 (is_u8 = 1, converted
 * to float without scaling); uv [n_points][2] in the OBJ convention; image_of_point [n_points] int32 (clamped to [0, n_images)).
 *   x = u * A - 0.5;  y = (1 - v) * A - 0.5;  x0 = floor(x), fx = x - x0;  y0 = floor(y), fy = y - y0;
 *   columns clamp(x0, 0, A-1) and clamp(x0 + 1, 0, A-1), rows likewise:  t00 = (x0, y0), t10 = (x0 + 1, y0), t01 = (x0, y0 + 1), t11;
 *   out = ((1 - fx) * t00 + fx * t10) * (1 - fy) + ((1 - fx) * t01 + fx * t11) * fy        -> out [n_points][C] fp32.
 *
 * Plain vector stores, no atomics, no random draws: the same bits from run to run, whatever the batch or the stream.  One launch each.
 * A count <= 0 returns 0 and launches nothing; hipErrorInvalidValue for texels outside 4..32, an atlas that is not a power of two in
 * 64..8192, rows outside [0, A], n_axis < 2, image_stride < rows A, channels outside 1..16, more than 65535 images, a NULL pointer or a
 * misaligned atlas.                                                                                                              */
int sc_texture_queries(const float* verts, const int32_t* faces, const long long* v_start, const long long* f_start,
                       const long long* f_count, int n_images, long long n_verts, long long n_faces, int atlas, int texels, double lo,
                       double hi, int n_axis, int rows, long long image_stride, float* query, int32_t* face_of_texel, void* stream);
int sc_texture_pack(const float* rgb, const float* normal, const int32_t* face_of_texel, int n_images, int atlas, int rows,
                    unsigned char* atlas_rgb, unsigned char* atlas_normal, void* stream);
int sc_texture_sample(const void* atlas_data, int is_u8, const float* uv, const int32_t* image_of_point, long long n_points,
                      int n_images, int atlas, int channels, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Triangle rasteriser (csrc/mesh_raster.hip): the indexed marching-cubes mesh seen from n_views cameras per image -- nearest face,
 * camera depth and perspective-correct barycentrics at every pixel centre (eval_3D.mesh_render, `--eval.mesh_render`).  Float
 * arithmetic is fp32, every operation rounded once (no contraction), division correctly rounded; coverage is exact integer arithmetic.
 * tests/mesh_raster_ref.py restates every line below in numpy.
 *
 * Inputs: verts [n_verts][3] fp32 in world units; faces [n_faces][3] int32, vertex numbers local to their image; v_start, f_start,
 * f_count [n_images] int64 on the device as for sc_texture_queries: image b's faces are faces[f_start[b] .. f_start[b] + f_count[b]),
 * its vertices are verts[v_start[b] .. v_end), v_end = v_start[b + 1] (n_verts for the last image), v_start non-decreasing.  A vertex
 * number is clamped into the image's range [0, v_end - v_start[b]) (and no access leaves verts); the caller keeps f_start + f_count <=
 * n_faces and the images' face ranges disjoint.  pose [n_images][n_views][3][4] world-to-camera, rows (r00 r01 r02 t0), ...: the
 * convention of camera.world2cam; intr [n_images][3][3], of which k00, k02, k11, k12 are read -- the skew k01 and k22 are not.
 *
 * Per vertex (x, y, z) and view, once:
 *   xc = ((r00 x + r01 y) + r02 z) + t0,  yc and zc likewise with rows 1 and 2;
 *   sx = (k00 * xc) / zc + k02,  sy = (k11 * yc) / zc + k12     (x to the right, y downward; pixel (i, j), column i and row j, has
 *        its centre at (i + 0.5, j + 0.5): camera.pixel_centers);
 *   X = (long long)rintf(sx * 256.0f),  Y = (long long)rintf(sy * 256.0f): the 1/256-pixel lattice, ties to even; a pixel centre is
 *        (256 i + 128, 256 j + 128).
 *   The vertex is `near` when zc < near (a NaN is not), else `out of range` when zc, sx * 256 or sy * 256 is not finite or |X| or
 *   |Y| >= 2^28.
 * Per face and view: dropped whole -- there is no clipping -- and counted in stats[1] when one of its vertices is near, else in
 * stats[2] when one is out of range.  With a, b, c its vertices on the lattice
 *   area = (bx - ax)(cy - ay) - (by - ay)(cx - ax)   in int64 (every edge function here is below 2^60);
 *   area == 0: dropped, stats[3];  area < 0: b and c swap, with their depths and barycentric slots, and area = -area (two-sided
 *   rendering); every other face is drawn, stats[0], whether or not it covers a pixel.
 *   For each edge p -> q of the oriented triangle (a -> b, b -> c, c -> a), d = q - p and a pixel centre P:
 *        E = dx (Py - py) - dy (Px - px)   in int64;  the edge holds P iff E > 0, or E == 0 and (dy < 0, or dy == 0 and dx > 0)
 *   (the top-left rule: a centre on an edge shared by two faces, or on a vertex shared by a fan, belongs to exactly one of them);
 *   the face covers P iff all three edges hold it.  Only centres inside the bounding box of the three lattice points and inside the
 *   image are looked at.
 *   With E_k the edge function opposite oriented vertex k (E_0 of b -> c, E_1 of c -> a, E_2 of a -> b; E_0 + E_1 + E_2 = area):
 *        b_k = (float)E_k / (float)area;  q_k = b_k / z_k;  s = (q_0 + q_1) + q_2  (oriented order);  depth = 1.0f / s;
 *        bary_k = q_k / s, stored in the slot of the face's own vertex (slots 1 and 2 swap back when b and c were swapped).
 * Visibility: the pixel goes to the smallest (bits(depth) << 32) | face, a 64-bit integer atomicMin (depth > 0, so bit order is value
 * order): the nearest face, on an exact tie the lowest face index.  A resolve pass, one thread per pixel, computes depth and bary
 * of the winning face again and writes the outputs; there are no float atomics and the outputs are the same bits from run to run.
 *
 * Two coverage paths that agree bit for bit (one device function evaluates a pixel for both): a face whose clamped box holds at
 * most large_pixels pixel centres is walked by its own thread; a larger one goes onto its (image, view)'s list through an integer
 * atomic cursor and is walked by one wave, lanes striding over the box.  large_pixels <= 0: every face by a wave.
 *
 * Outputs, [n_images][n_views][height][width] row-major: face int32 (local face number, -1 where no face covers the centre), depth
 * fp32 (camera z, 0 on a miss), bary [..][3] fp32 (0 on a miss); stats [n_images][n_views][4] int32 = faces drawn, culled by near,
 * culled by range or not finite, of zero area.  Every element is written.  scratch: sc_mesh_raster_scratch_bytes(...) bytes,
 * 16-byte aligned (keys, projected vertices [n_views][n_verts] of 16 B, lists, cursors); the query returns -1 for sizes the call
 * refuses.  Three memsets and four launches on the caller's stream, plain vector stores, no host synchronisation.
 * n_images, n_verts or n_faces <= 0 returns 0 and launches nothing (the outputs are not written); hipErrorInvalidValue for height or
 * width outside 1..4096, n_views outside 1..65535, near <= 0 (or NaN), more than 65535 images, more than 2^31 vertices or faces, more
 * than 2^40 output pixels, a NULL pointer or a misaligned scratch.                                                              */
long long sc_mesh_raster_scratch_bytes(int n_images, int n_views, long long n_verts, long long n_faces, int height, int width);
int sc_mesh_raster(const float* verts, const int32_t* faces, const long long* v_start, const long long* f_start,
                   const long long* f_count, const float* pose, const float* intr, int n_images, long long n_verts, long long n_faces,
                   int n_views, int height, int width, float near, long long large_pixels, int32_t* face, float* depth, float* bary,
                   int32_t* stats, void* scratch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ambient occlusion from the level grid (csrc/level_ao.hip): how much of the hemisphere over a surface point is free of the solid
 * {level < iso} within a reach of n_steps * step grid pitches (ops.level_ambient_occlusion, `--mesh.ao`).  The grid is the solid:
 * there is no triangle and no tree.  All arithmetic is fp32, every operation rounded once (no contraction), division correctly
 * rounded; tests/level_ao_ref.py restates every line below in numpy and the GPU tests compare bit for bit.
 *
 * Inputs: level [n_images][S][S][S] fp32, index (x S + y) S + z, S = n_axis in 2..1024; points [n_points][3] fp32 in grid-index units
 * (the units of sc_marching_cubes_mesh's vertices); normals [n_points][3] fp32, any length; image [n_points] int32, the image a
 * point belongs to; dirs [64][3] fp32, the directions, which are data (ops.ao_directions: a Fibonacci set built in float64 on the host
 * and rounded once -- the device evaluates no sine); step, bias, iso fp32; n_steps = M in 1..4096.
 *
 * Per point (p, n) and direction k, D = dirs[k]:
 *   dn = (D.x n.x + D.y n.y) + D.z n.z;   d = -D if dn < 0, else D (the direction folded into the normal's hemisphere);   w = |dn|;
 *   p0_c = p_c + bias * n_c   for c = x, y, z;
 *   for s = 1 .. M:   t = (float)s * step;   q_c = p0_c + t * d_c;
 *       the ray ends OPEN when !(q_c >= 0 && q_c <= (float)(S - 1)) for any c (the negated form: a NaN ends the ray as well);
 *       i_c = min((int)floorf(q_c), S - 2);   f_c = q_c - (float)i_c;   the sample's cell is (i_x, i_y, i_z), its corners
 *       v[a][b][c] = level[image][i_x + a][i_y + b][i_z + c];
 *       if no corner is < iso the sample cannot occlude and the march goes on -- a rule, not an optimisation: it makes skipping
 *       a cell that a bit volume calls empty exact;
 *       else, with lerp(a, b, t) = a + t * (b - a):   u[a][b] = lerp(v[a][b][0], v[a][b][1], f_z);
 *       u[a] = lerp(u[a][0], u[a][1], f_y);   val = lerp(u[0], u[1], f_x);   the ray ends CLOSED when val < iso;
 *   a ray that no sample ended is OPEN.
 *   W = the sum over the 64 directions of w, V = the sum of (open ? w : 0), both by the fixed pairwise tree a[j+1][k] = a[j][2k] +
 *   a[j][2k+1], j = 0..5, which is what lane 0 holds after a __shfl_xor butterfly over the masks 1, 2, 4, 8, 16, 32.
 *   ao = V / W;   mask = the open bits, bit k for direction k.
 *   A point or normal with a component that is not finite, or !(W > 0) (a zero normal; a NaN), gives ao = 1 and mask = -1.
 *   An image outside 0 .. n_images - 1 sets *bad to 1, gives ao = 1 and mask = -1 and reads nothing of level.
 *
 * One wave64 is one point and one lane one direction: __ballot is the mask.  cell_skip != 0: a first launch writes, per image, the
 * bit volume of the cells with a corner < iso -- [S-1][S-1][ceil((S-1) / 32)] uint32 words, bit z & 31 of word z >> 5 of row (x, y),
 * one thread per word, plain stores -- into scratch, and the march tests a sample's bit before it loads the 8 corners;
 * cell_skip == 0: scratch is not used and the corner test comes from the loads.  The same bits either way.
 * Outputs: ao [n_points] fp32, mask [n_points] int64, bad [1] int32 (zeroed here); every element is written.  scratch:
 * sc_level_ao_scratch_bytes(n_images, n_axis) bytes, 4-byte aligned (-1 for sizes the call refuses).  One memset and one or two
 * launches on the caller's stream; no atomics, no LDS, no host synchronisation.  n_points <= 0 returns 0 and launches nothing.
 * hipErrorInvalidValue for n_axis outside 2..1024, n_steps outside 1..4096, n_images outside 1..65535, more than 2^30 points, a NULL
 * pointer (scratch may be NULL when cell_skip == 0).                                                                            */
#define SC_LEVEL_AO_DIRS 64
#define SC_LEVEL_AO_MAX_STEPS 4096
long long sc_level_ao_scratch_bytes(int n_images, int n_axis);
int sc_level_ambient_occlusion(const float* level, const float* points, const float* normals, const int32_t* image, const float* dirs,
                               int n_images, int n_axis, long long n_points, float step, float bias, float iso, int n_steps,
                               int cell_skip, void* scratch, float* ao, long long* mask, int32_t* bad, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Launch policy (csrc/device.hip) -- the one process-level setting of the library. The persistent one-workgroup-per-CU grids
 * (stream-K 3x3 convolutions and their weight gradients, stem / 1x1 / stride-2 gradients) are sized for
 * sc_grid_cus() = device CUs - reserved.  Reserve CUs when another stream must make progress beside them: RCCL's
 * all-reduce kernels in a multi-GPU step (the reference leaves this to DDP / NCCL: model/runner.py:121).  Call before sizing
 * workspaces (the *_workspace_floats queries follow the grid); default 0, or SHAPECLIPPER_RESERVE_CUS.  Host-only calls.       */
int sc_set_reserved_cus(int n);
int sc_grid_cus(void);
/* The convolution launches keep one small device table per (device, shape, grid) -- the stream-K span cut -- created by the first launch
 * of a shape outside a stream capture (stream-ordered copy on the launch stream).  This frees them all (rebuilt on demand); call
 * with no convolution in flight.                                                                                               */
int sc_conv3x3_release_tables(void);
/* The work partition a 3x3 convolution launch follows (conv_plan / conv_span_cut in csrc/conv3x3.hip, which the launches themselves
 * read): host only, launches nothing.  family 0: sc_conv3x3_forward, 1: sc_conv3x3_forward_split, 2: sc_conv3x3s2_forward,
 * 3: sc_conv3x3s2_backward_data; hw, batch, cin, cout as that entry point takes them (family 2 / 3: hw = side of the forward INPUT
 * map, cin / cout of the forward convolution).  cus: compute units of the persistent grid, cus <= 0 asks sc_grid_cus() (the only
 * device call); equal_spans != 0: the cut a launch uses when it has no span table (first launch of a shape under a stream capture).
 * The rule: a tile is CT output channels x PT consecutive flat output pixels (x 4 parity phases, family 3), its reduction nk K-steps
 * of 8 channels (family 1: rounded up to even).  G = workgroups.  Workgroup g computes the tiles r G + perm(g), r < rounds = tiles / G,
 * whole, with perm(g) = (x < G % 8 ? x (G / 8 + 1) : (G % 8) (G / 8 + 1) + (x - G % 8) (G / 8)) + g / 8, x = g % 8 (one contiguous
 * range of a round per XCD).  The K-steps of the other tail_tiles = tiles % G tiles, in tile-major order, are cut into G spans
 * [spans[g], spans[g + 1]) of at most nk steps -- greedy at the smallest bound on 2 steps + ov2 tiles touched that G spans cover, or
 * equal spans of per_wg = ceil(tail_tiles nk / G) -- and the fix-up launch adds the partial tiles of a shared tile in K order; a tail
 * tile that one span covers exactly is stored by its workgroup and skipped by the fix-up.
 * plan[10] (host memory) = { tiles, nk, rounds, tail_tiles, per_wg, PT, CT, ov2, G, 1 if the spans are the table's else 0 };
 * spans[G + 1] (host memory, may be NULL; size it with a first call) = the span starts, spans[G] = tail_tiles nk.
 * Refuses what the launch refuses (hipErrorInvalidValue; -1 for a map side the family does not have), and a NULL plan.          */
int sc_conv3x3_plan(int family, int hw, int batch, int cin, int cout, int cus, int equal_spans, int* plan, int* spans);

#ifdef __cplusplus
}
#endif
#endif
