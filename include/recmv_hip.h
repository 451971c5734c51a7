/*
 * recmv_hip.h — C ABI of librecmv_hip.so, the MI355X (gfx950) implementation of the
 * REC-MV per-frame implicit-surface optimisation hot path.
 *
 * This is the drop-in boundary: every entry point replaces one function of the reference's
 * pybind11/CUDA extensions (FastMinv, MCGpu, GridSamplerMine, interp2x_boundary3d) or one dense
 * contraction that the reference leaves to torch/cuBLAS inside its nn.Modules.  Plain pointers and
 * sizes only — no torch types.  All pointers are DEVICE pointers unless the name says `host`.
 * `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  Every function
 * returns RECMV_OK (0) or a negative RECMV_ERR_* code; recmv_last_error() gives a message for the
 * calling thread.  The library never allocates caller-visible memory; marching cubes is two-phase
 * (count -> caller allocates -> emit) and keeps a caller-provided workspace.
 *
 * Reference citations are relative to the REC-MV tree.
 */
#ifndef RECMV_HIP_H_
#define RECMV_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RECMV_OK               0
#define RECMV_ERR_ARG         -1   /* bad argument (NULL pointer, negative size, unsupported mode) */
#define RECMV_ERR_HIP         -2   /* a HIP runtime call or kernel launch failed                  */
#define RECMV_ERR_UNSUPPORTED -3   /* combination not implemented (e.g. dtype)                    */
#define RECMV_ERR_WORKSPACE   -4   /* caller workspace too small                                  */

#define RECMV_F32 0
#define RECMV_F64 1

/* ABI version, bumped when an existing signature changes (recmv/_lib.py checks the number at load).
 *   v11: the mesh-grid entry points take a recmv_mesh_grid descriptor in place of the grid's loose arguments
 *        (recmv_mesh_grid_count / _fill, recmv_closest_point_grid, recmv_mesh_intersect_grid_count / _fill,
 *        recmv_segment_mesh_grid).  Added since without a bump: recmv_icp_accumulate and its workspace size;
 *        recmv_graph_components, recmv_mesh_face_stats, recmv_segment_sums with its chunk and workspace sizes;
 *        recmv_vertex_quadrics, recmv_edge_collapse_cost, recmv_collapse_flip_check; recmv_cotan_weights,
 *        recmv_laplacian_step, recmv_face_normal_filter, recmv_vertex_from_normals (mesh smoothing: pure additions, still v11);
 *        recmv_points_within_cells, recmv_points_within_count, recmv_points_within_fill, recmv_points_within_max_cells (the
 *        point-pair search of mesh repair: pure additions, still v11); recmv_voxel_band_workspace_bytes,
 *        recmv_voxel_band_distance, recmv_voxel_sign_fill with the recmv_lattice descriptor (mesh voxelisation: pure additions,
 *        still v11); recmv_hole_triangulate, recmv_hole_triangulate_workspace_bytes, recmv_hole_fill_lds_max_edges,
 *        recmv_hole_fill_auto_max_edges, recmv_hole_fill_max_edges (hole filling: pure additions, still v11);
 *        recmv_winding_chunk_faces, recmv_winding_exact_workspace_bytes, recmv_winding_exact, recmv_winding_tree_nodes,
 *        recmv_winding_tree_cells, recmv_winding_tree_build, recmv_winding_tree_query with the recmv_winding_tree descriptor
 *        (generalized winding numbers: pure additions, still v11); recmv_geodesic_lds_max_vertices,
 *        recmv_geodesic_auto_max_vertices, recmv_geodesic_workspace_bytes, recmv_geodesic_check_sources, recmv_geodesic_sweeps,
 *        recmv_geodesic_lds (geodesic distance fields: pure additions, still v11); recmv_param_lds_max_vertices,
 *        recmv_param_auto_max_vertices, recmv_param_solve_workspace_bytes, recmv_param_solve, recmv_param_solve_lds,
 *        recmv_param_face_frames, recmv_param_arap_rhs, recmv_param_distortion (mesh parameterisation: pure additions, still v11);
 *        recmv_bake_raster, recmv_bake_gutter, recmv_bake_pad, recmv_bake_interpolate, recmv_bake_transfer,
 *        recmv_bake_vertex_tangents, recmv_bake_encode_normal (texture baking: pure additions, still v11).
 *   v10: recmv_verts_normals, recmv_hard_phong_shade, recmv_hard_phong_params_floats added.  Added since without a bump (no
 *        existing signature changed, and _lib.py rejects a library that lacks them): recmv_knn1, recmv_nricp_energy,
 *        recmv_lap_align_solve, recmv_lap_smooth, recmv_closest_point, recmv_iso_relax, recmv_loop_subdivide,
 *        recmv_point_mesh_nearest, recmv_collision_push, recmv_curve_tubes, recmv_curve_fit_step, the mesh-grid entry points,
 *        recmv_mesh_intersect_brute, recmv_segment_mesh_brute and their workspace sizes.
 *   v9: recmv_lbs_jet_* added.  v8: recmv_cam_* added.  v7: recmv_get_sampler_mode, recmv_set_jet_fill added.
 *   v6: recmv_def_regu, recmv_b3_*, recmv_mlp_rows_*, recmv_mc_run_batch added.  v5: second weight set + split_row in recmv_mlp. */
int recmv_abi_version(void);
/* 1 when every kernel of the library was built without packed-f32 VALU instructions (RECMV_NO_PACKED_F32=1 at build time): the build
 * the optional bf16x6 matrix mode needs — beside its NT product kernels, waves executing v_pk_*_f32 were caught computing wrong values in
 * lanes 48-63.  (ABI v7) */
int recmv_no_packed_f32(void);
/* Message of the last error on this thread ("" if none). */
const char* recmv_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * A. FastMinv — batched 3x3 inverse.
 *   replaces Fast3x3Minv            (FastMinv/M3x3Inv.cpp:12-36, kernel Matrix3x3InvKernels.cu:22-61)
 *            Fast3x3Minv_backward   (FastMinv/M3x3Inv.cpp:38-59, kernel Matrix3x3InvKernels.cu:64-104)
 * ms/invs/grads/outs: [n,3,3] contiguous, dtype f32|f64.  checks: [n] bytes (0/1) == torch.bool.
 * Singular rule: fabs(det) < 1e-4 (absolute) -> inverse = 0, check = 0.
 * ---------------------------------------------------------------------------------------------- */
int recmv_inv3x3_forward(const void* ms, void* invs, uint8_t* checks, int64_t n, int dtype, void* stream);
int recmv_inv3x3_backward(const void* grads, const void* invs, void* outs, int64_t n, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * A2. Deformation regulariser of the render loss: value and gradient of GM(sum_i log^2 sigma_i(J)) per matrix.
 *   replaces the host SVD + its autograd of OptimGarmentNetwork.py:1143-1155
 *            (Jacobs.cpu() -> torch.svd -> log -> utils.GMRobustError(., def_regu.c, True), utils/utils.py:87-91).
 * J: [P,3,3] contiguous f32 (Jacobian of the offset MLP at the sampled points).  y: [P] = 2 x / c^2 / (x / c^2 + 4) with
 * x = sum_i log^2 sigma_i;  gJ: [P,3,3] = dy/dJ (singular values below 1e-10 are clamped there: value from the bound, no gradient).
 * The caller takes the mean and scales gJ in its backward pass.
 * ---------------------------------------------------------------------------------------------- */
int recmv_def_regu(const float* J, int64_t P, float c, float* y, float* gJ, void* stream);

/* ------------------------------------------------------------------------------------------------
 * A3. Camera of the loop (ABI v8): world points -> image coordinates, pixels -> world rays, with their backward passes.
 *   replaces the element-wise torch chains of RectifiedPerspectiveCameras, model/CameraMine.py:62-88 + 281-300 (the calibration
 *            matrix behind transform_points: fx' = fx / (W/2), px' = 1 - 1/W - px / (W/2)), :104-142 (transform_points_screen),
 *            :146-169 (view_rays) and `project`.
 * cam16: 16 device floats = R [3][3] row-major (world -> view: v = p R + T), T [3], focal length (fx, fy), principal point (px, py).
 * W, H: image size in pixels.  mode: 0 -> out [P,3] = (x_ndc, y_ndc, z_view); 1 -> out [P,3] = (screen_x, screen_y, 1 / z_view),
 *   screen = (S - 1) / 2 - S * ndc / 2; 2 -> out [P,2] = pixel (px - x fx / z, py - y fy / z).
 * Backward: g_pts [P,3] (may be NULL) and g_cam7 = d/d(T[3], focal[2], principal point[2]) summed over the points in a FIXED order
 *   (per-workgroup partial sums into `partial`, recmv_cam_partial_floats(P) floats owned by the caller, then one pass over them):
 *   bit-reproducible, no float atomics.  R gets no gradient (the loop's camera rotation is not optimised).
 * Rays: pixel (x, y, w) as [P,3] floats in `pix`, or — pix NULL — integer (col, row) with w = 1 -> unit world ray
 *   normalize(-x / fx + w px / fx, -y / fy + w py / fy, w) R^T; backward: g_cam4 = d/d(focal[2], principal point[2]).
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_cam_partial_floats(int64_t P);
int recmv_cam_project(const float* pts, int64_t P, const float* cam16, float W, float H, int mode, float* out, void* stream);
int recmv_cam_project_backward(const float* pts, const float* g_out, int64_t P, const float* cam16, float W, float H, int mode,
                               float* g_pts, float* g_cam7, float* partial, int64_t partial_floats, void* stream);
int recmv_cam_rays(const float* pix, const int64_t* col, const int64_t* row, int64_t P, const float* cam16, float* out, void* stream);
int recmv_cam_rays_backward(const float* pix, const int64_t* col, const int64_t* row, const float* g_out, int64_t P,
                            const float* cam16, float* g_cam4, float* partial, int64_t partial_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * C. GridSamplerMine — 3-D trilinear sampler, padding=border, align_corners=False, with first and
 * second derivative.
 *   replaces GridSamplerMine.forward / backward / dbackward
 *            (MCAcc/cuda/GridSamplerMine.cpp:73-96; kernels GridSamplerMineKernel.cu:162-328,
 *             333-570, 575-914).
 * Tensors are described by sizes/strides in ELEMENTS (like the reference's TensorInfo), so any
 * strided layout is accepted.  input: [N,C,D,H,W]; grid: [N,Do,Ho,Wo,3]; output/grad_output:
 * [N,C,Do,Ho,Wo].  A channels-last input (stride[1]==1) with contiguous grid takes the vectorised
 * fast path.  interp must be 0 (bilinear) and pad 1 (border), as in the reference's check()
 * (GridSamplerMine.cpp:58-63) — anything else returns RECMV_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------------- */
typedef struct recmv_tensor5 {
  int64_t size[5];
  int64_t stride[5];
} recmv_tensor5;

int recmv_grid_sample3d_forward(const void* input, const recmv_tensor5* input_desc,
                                const void* grid, const recmv_tensor5* grid_desc,
                                void* output, const recmv_tensor5* output_desc,
                                int interp, int pad, int dtype, void* stream);

/* grad_input may be NULL: the scatter into the (frozen) volume is skipped — the hot path's volume
 * is a registered buffer, never a parameter (model/Deformer.py:240-243).  When non-NULL it must be
 * zero-filled by the caller (the reference zero-fills it itself: GridSamplerMineKernel.cu:955).
 * grad_grid: [N,Do,Ho,Wo,3] contiguous (the reference assumes this too: ...Kernel.cu:538-545). */
/* Summation order of backward / double backward when only grad_grid (and grad_grad_output) are asked for on a channels-last f32
 * volume: 0 (default) = record-coalesced lanes — G lanes per point, per-point sums finished by a lane butterfly: the reference's
 * terms in a different order, within a few ulp of sum |terms| (north_star: gradients within an f32 tolerance); 1 = one lane per
 * point with the channel loop in the reference's order (GridSamplerMineKernel.cu:333-914), bit-equal to the oracle.  Requests
 * with grad_input or ggI, f64, or other layouts always take the exact kernels.  Returns the previous mode. */
int recmv_set_sampler_mode(int mode);
/* The mode in force, read without changing it (ABI v7; GridSamplerMine.current_mode of the Python side reads it at forward time). */
int recmv_get_sampler_mode(void);

int recmv_grid_sample3d_backward(const void* input, const recmv_tensor5* input_desc,
                                 const void* grid, const recmv_tensor5* grid_desc,
                                 const void* grad_output, const recmv_tensor5* grad_output_desc,
                                 void* grad_input, const recmv_tensor5* grad_input_desc,
                                 void* grad_grid,
                                 int interp, int pad, int dtype, void* stream);

/* Double backward.  ggI = grad wrt backward's grad_input output (layout like input; may be NULL ->
 * treated as zeros), ggG = grad wrt backward's grad_grid output ([N,Do,Ho,Wo,3], strided).
 * Outputs: grad_input (like input; NULL to skip; caller zero-fills), grad_grid (contiguous),
 * grad_grad_output (like grad_output; written, not accumulated). */
int recmv_grid_sample3d_dbackward(const void* ggI, const recmv_tensor5* ggI_desc,
                                  const void* ggG, const recmv_tensor5* ggG_desc,
                                  const void* input, const recmv_tensor5* input_desc,
                                  const void* grid, const recmv_tensor5* grid_desc,
                                  const void* grad_output, const recmv_tensor5* grad_output_desc,
                                  void* grad_input, const recmv_tensor5* grad_input_desc,
                                  void* grad_grid,
                                  void* grad_grad_output, const recmv_tensor5* grad_grad_output_desc,
                                  int interp, int pad, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * C2. interp2x_boundary3d — (2n-1) trilinear upsample + boundary mask.
 *   replaces interp2x_boundary3d.forward / backward
 *            (MCAcc/cuda/interp2x_boundary3d.cpp:17-37; kernels interp2x_boundary3d_kernel.cu:11-239)
 * input: [B,C,d,h,w] contiguous -> output [B,C,2d-1,2h-1,2w-1], is_boundary same shape (bytes).
 * ---------------------------------------------------------------------------------------------- */
int recmv_interp2x_boundary3d_forward(const void* input, void* output, uint8_t* is_boundary,
                                      int64_t bc, int64_t d, int64_t h, int64_t w,
                                      float balance_value, int dtype, void* stream);
/* grad_output: [B,C,D,H,W] contiguous (D,H,W odd) -> grad_input [B,C,(D+1)/2,(H+1)/2,(W+1)/2]. */
int recmv_interp2x_boundary3d_backward(const void* grad_output, void* grad_input,
                                       int64_t bc, int64_t D, int64_t H, int64_t W,
                                       int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E. MCGpu — marching cubes on an x-major f32 volume sdf[NX][NY][NZ] (index i*NY*NZ+j*NZ+k).
 *   replaces MCGpu.mc_gpu (MCGpu/MCGpu.cpp:20-56; MCGpu::init/MC/scaleVertices
 *            MCGpu/CudaKernels.cu:572-639; kernels :316-521).
 * Deterministic: vertices ordered by edge key ((x*NY+y)*NZ+z)*3+dir, faces by (voxel, triangle#),
 * corner order reversed exactly as the reference (CudaKernels.cu:502).  An edge whose owner voxel is
 * outside the grid has no vertex and is referenced as -1, as in the reference.
 *
 * recmv_mc_run is the whole extraction on the stream with NO host round trip (the reference reads its counters
 * back between its two kernels, CudaKernels.cu:628): the caller passes output buffers with capacities, the
 * kernels never write past them, and `counts_device` (3 x int32 {n_vertices, n_faces, n_active_voxels}, DEVICE
 * pointer) receives the true sizes — if one exceeds its capacity the caller re-allocates and calls
 * recmv_mc_emit with the same workspace (the classification is still in it).
 * Two-phase form: recmv_mc_count classifies + scans and returns the sizes through `counts_host` (HOST pointer,
 * written after an internal stream sync — the same D2H round trip as the reference's); the caller allocates
 * vertices [V,3] f32 and faces [F,3] i64 and calls recmv_mc_emit with the same workspace and n_active_voxels
 * (the number of voxels that own a vertex or a triangle: recmv_mc_emit runs one lane per such voxel from the
 * list the scan left in the workspace).
 * recmv_mc_workspace_bytes gives the workspace size for a volume (0 if the volume is not supported).
 * Limits: at most 2^28 lattice points, every dimension < 32768.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int recmv_mc_count(const float* sdf, int64_t nx, int64_t ny, int64_t nz, float iso,
                   void* workspace, int64_t workspace_bytes, int32_t* counts_host, void* stream);
int recmv_mc_emit(const float* sdf, int64_t nx, int64_t ny, int64_t nz, float iso,
                  float xstep, float ystep, float zstep, float xmin, float ymin, float zmin,
                  const void* workspace, int64_t workspace_bytes, int64_t n_active_voxels,
                  float* vertices, int64_t vertex_capacity, int64_t* faces, int64_t face_capacity, void* stream);
int recmv_mc_run(const float* sdf, int64_t nx, int64_t ny, int64_t nz, float iso,
                 float xstep, float ystep, float zstep, float xmin, float ymin, float zmin,
                 void* workspace, int64_t workspace_bytes,
                 float* vertices, int64_t vertex_capacity, int64_t* faces, int64_t face_capacity,
                 int32_t* counts_device, void* stream);
/* The same for up to 4 volumes of ONE lattice size in one set of four launches (grid y = volume): the three nets of a re-mesh —
 * body + two garments, engineer/networks/OptimGarmentNetwork.py:581-618 calls MCGpu.mc_gpu once per net — share every launch; the
 * passes after the volume stream work on kilobytes and are launch-latency bound.  sdf / workspaces / vertices / faces /
 * counts_device: HOST arrays of n device pointers (every volume its own workspace of recmv_mc_workspace_bytes); capacities per
 * volume; results per volume exactly those of recmv_mc_run. */
int recmv_mc_run_batch(int n, const float* const* sdf, int64_t nx, int64_t ny, int64_t nz, float iso, float xstep, float ystep,
                       float zstep, float xmin, float ymin, float zmin, void* const* workspaces, int64_t workspace_bytes,
                       float* const* vertices, const int64_t* vertex_capacity, int64_t* const* faces,
                       const int64_t* face_capacity, int32_t* const* counts_device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E'. Seg3dLossless bookkeeping on the device (csrc/seg3d.hip) — the per-level steps of
 *   MCAcc/seg3d_lossless.py:_forward (:233-428) between the upsampler (C above) and the MLP queries: which voxels of
 *   the level to query, their world points, the write-back with sign-conflict detection, and the growth of the
 *   conflicts' 3^3 neighbourhoods.  Volumes are [D,H,W], x fastest, linear voxel index i = (z*H + y)*W + x (int32);
 *   the set of evaluated voxels is a bit volume (uint32 words, bit i&31 of word i>>5; ceil(D*H*W/32)+1 words).
 *   Every counter is a DEVICE int32 that the call zeroes first; lists are never written past `capacity`.
 *   recmv_seg3d_select : list = voxels with dilate3x3x3(is_boundary) != 0 that are not evaluated, where "evaluated" =
 *                        bit of the parent level (sizes (D+1)/2 ...) at even coordinates; `done` receives
 *                        evaluated | listed for the whole level (replaces: box filter, coords_accum erase, transposed
 *                        nonzero, unique(dim=1) of :296-330).  List order is unspecified.
 *   recmv_seg3d_points : points[t] = ((x*sx, y*sy, z*sz) / res + (1/res)/2) * extent + bmin  (batch_eval, :99-101)
 *   recmv_seg3d_apply  : flags[t] = (occupancy[i] - balance) * (values[t] - balance) < 0, then occupancy[i] = values[t]
 *   recmv_seg3d_expand : list_out = not-yet-evaluated voxels of the 3^3 blocks (clamped to the grid) around the flagged
 *                        voxels, each exactly once; their bits are set in `done` (:348-372 without unique(dim=0))
 * ---------------------------------------------------------------------------------------------- */
int recmv_seg3d_select(const uint8_t* is_boundary, const uint32_t* done_prev, int64_t D, int64_t H, int64_t W,
                       uint32_t* done, int32_t* list, int64_t capacity, int32_t* count_device, void* stream);
int recmv_seg3d_points(const int32_t* list, int64_t n, int64_t H, int64_t W, const int32_t* stride_xyz,
                       const float* res_xyz, const float* extent_xyz, const float* bmin_xyz, float* points,
                       void* stream);
int recmv_seg3d_apply(const int32_t* list, const float* values, int64_t n, float balance, float* occupancy,
                      uint8_t* conflict_flags, int32_t* conflict_count_device, void* stream);
int recmv_seg3d_expand(const int32_t* list, const uint8_t* conflict_flags, int64_t n, int64_t D, int64_t H, int64_t W,
                       uint32_t* done, int32_t* list_out, int64_t capacity, int32_t* count_device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * A/B/D. Dense f32 contractions of the three MLPs (SDF model/network.py:98-111, deformer
 * model/Deformer.py:194-199, colour model/RenderNet.py:83-94) — torch.nn.Linear/cuBLAS sgemm in the
 * reference.  f32 MFMA (v_mfma_f32_32x32x2_f32), exact-f32 accumulate.
 *
 *   recmv_gemm_nt :  C[M,N] = act( alpha * (A[M,K] . B[N,K]^T) + bias[N] ) * out_scale
 *   recmv_gemm_tn :  C[M,N] = A[K,M]^T . B[K,N]      (weight gradients: reduction over points)
 *
 * lda/ldb/ldc are row strides in elements.  act: RECMV_ACT_*.  `bias` may be NULL.
 * For softplus the reference's nn.Softplus(beta=100) semantics are used (threshold 20).
 * recmv_gemm_tn needs a workspace of recmv_gemm_tn_workspace_bytes() for its split-K partials.
 * ---------------------------------------------------------------------------------------------- */
#define RECMV_ACT_NONE     0
#define RECMV_ACT_RELU     1
#define RECMV_ACT_SOFTPLUS 2   /* softplus(beta), param = beta */
#define RECMV_ACT_TANH     3

int recmv_gemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias,
                  float* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                  int act, float act_param, float out_scale, void* stream);
/* C[M,N] = ( G (.) act'(z) * g_scale ) . B^T with act'(z) taken through y = act(z) = y_scale * Y[m,k]: the
 * activation-gradient step of a layer's backward fused into the A-operand staging of the dX product.
 * ldg may be 0 (one cotangent row shared by all points). */
int recmv_gemm_nt_actgrad(const float* G, int64_t ldg, const float* Y, int64_t ldy, const float* B, int64_t ldb,
                          float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int act, float act_param,
                          float y_scale, float g_scale, void* stream);
/* C[M,N] = (A . B^T) (.) act'(y_scale * Y) * scale with Y [M,N] (row stride ldy): the activation-gradient step of the
 * NEXT layer of a backward chain applied in the epilogue of the product that creates its cotangent — each element
 * once (recmv_gemm_nt_actgrad, the operand-side fusion, recomputes it in every column tile). */
int recmv_gemm_nt_mulgrad(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                          int64_t N, int64_t K, const float* Y, int64_t ldy, int act, float act_param, float y_scale,
                          float scale, void* stream);
/* recmv_gemm_nt / recmv_gemm_nt_mulgrad over a row block that holds the rows of TWO nets of one shape (the two garments' SDF nets
 * in the surface root finder, utils/FindSurfacePs.py:273-353: one launch per layer for both): rows [0, split_row) multiply by
 * B (+ bias), rows [split_row, M) by B2 (+ bias2).  split_row must be a multiple of 128; B2 == NULL is the plain product. */
int recmv_gemm_nt_seg(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, const float* B2,
                      const float* bias2, int64_t split_row, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int act,
                      float act_param, float out_scale, void* stream);
int recmv_gemm_nt_mulgrad_seg(const float* A, int64_t lda, const float* B, const float* B2, int64_t split_row, int64_t ldb,
                              float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, const float* Y, int64_t ldy, int act,
                              float act_param, float y_scale, float scale, void* stream);
/* Matrix mode of recmv_gemm_nt (and everything built on it): 0 = f32-input MFMA, the default — bit-for-bit an f32
 * fma chain; 1 = "bf16x6": every f32 operand element is split into three bf16 pieces in registers and each tile step
 * issues the six bf16 MFMA products of weight >= 2^-18 with f32 accumulation (f32-level accuracy, up to 2.7x the f32
 * matrix rate).  Returns the previous mode. */
int recmv_set_gemm_mode(int mode);
int recmv_get_gemm_mode(void);
/* Mode 1 only: which kernel families compute in bf16x6 — bit 0 the 128 x 128 NT tiles, bit 1 the 64 x 64 / 64 x 32 NT tiles, bit 2 the
 * TN (dW) tiles; the others stay on the exact-f32 kernels.  7 (default) = all.  A bisect / A-B switch; returns the previous mask. (ABI v7) */
int recmv_set_b3_families(int mask);
/* How the jet pass (recmv_mlp_jet_forward) zeroes the code / padding columns of its tangent rows: 1 (default) = a kernel over those
 * columns only, 0 = hipMemsetAsync over the whole tangent block (rounds 1-4; the A/B of tools/loop_repro_inproc.py).  Same bits either
 * way.  Process-global; RECMV_JET_FILL_KERNEL=0 sets 0 at load.  Returns the previous value.  (ABI v7) */
int recmv_set_jet_fill(int use_kernel);
/* bf16x6 mode, weights split ONCE: recmv_b3_split writes the three bf16 planes [3][N][Kp] (Kp = K rounded up to 32, zero-padded) of
 * a weight matrix B [N][K] (row stride ldb, K % 8 == 0, 16-byte aligned rows) into `planes` (recmv_b3_planes_bytes(N, K) bytes,
 * owned by the caller) and remembers them under B's address; the large bf16x6 products (recmv_gemm_nt and everything built on it,
 * with this B, K and ldb, N rows or fewer) then read the pieces instead of splitting B's tile in every row tile — same pieces, same
 * products, same order: bit-identical results.  The caller keeps B's contents unchanged while the entry exists and calls
 * recmv_b3_forget(B) before B or `planes` is freed.  (The weights of the reference are nn.Linear parameters under weight_norm,
 * model/network.py:49-86: re-normalised once per pass, read by every product of the pass.) */
int64_t recmv_b3_planes_bytes(int64_t N, int64_t K);
int recmv_b3_split(const float* B, int64_t ldb, int64_t N, int64_t K, void* planes, int64_t planes_bytes, void* stream);
int recmv_b3_forget(const float* B);
int64_t recmv_gemm_tn_workspace_bytes(int64_t M, int64_t N, int64_t K);
/* C [M,N] = A^T B with A [K,M], B [K,N].  K = 0 (an empty reduction): C is zeroed; A, B, lda, ldb and the workspace are neither read nor
 * checked (may be NULL). */
int recmv_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb,
                  float* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* Positional encoding (model/Embedder.py:4-65): out[p, 0:3] = x, then for each of L frequency bands
 * 2^i: w[2i]*sin(2^i x), w[2i+1]*cos(2^i x) (3 values each).  out row stride ldo >= 3+6L; columns
 * [3+6L, ldo_fill) are zero-filled (ldo_fill <= ldo) so padded K reads as zeros; everything is
 * multiplied by out_scale (1/sqrt(2) for the skip connection, model/network.py:105-106).
 * weights: HOST pointer to 2L floats (utils/utils.py:40-46 produces python floats), or NULL = ones. */
int recmv_posenc_forward(const float* x, int64_t ldx, float* out, int64_t ldo, int64_t ldo_fill,
                         int64_t P, int L, const float* weights_host, float out_scale, void* stream);

/* Fused element-wise steps between the MFMA layers (csrc/elementwise.hip):
 *   recmv_act_grad  : out = gy * act'(z) written through y = act(z)     (backward of a fused layer)
 *   recmv_act_grad2 : out = a * b * d(act')/dy                           (its double backward)
 *   recmv_weight_norm_forward/backward : W = g * v/||v|| per output row (nn.utils.weight_norm dim 0,
 *                     model/network.py:82-85, model/RenderNet.py:47-50); norms [rows] is saved for backward. */
int recmv_act_grad(const float* gy, const float* y, float* out, int64_t n, int act, float act_param, void* stream);
int recmv_act_grad2(const float* a, const float* b, const float* y, float* out, int64_t n, int act, float act_param,
                    void* stream);
int recmv_weight_norm_forward(const float* v, const float* g, float* W, float* norms, int64_t rows, int64_t cols,
                              void* stream);
int recmv_weight_norm_backward(const float* v, const float* g, const float* norms, const float* gW, float* gv,
                               float* gg, int64_t rows, int64_t cols, void* stream);

/* Derivatives of the positional encoding (so that autograd of any order stays one launch):
 *   recmv_posenc_vjp : t == NULL -> out[P,3] = J(x)^T g               (g: [P, 3+6L], row stride ldg)
 *                      t != NULL -> out[P,3] = t * d/dx <g, J(x) 1>   (second-derivative term, see posenc_grad.hip)
 *   recmv_posenc_jvp : out[P, 3+6L] = J(x) t                          (t: [P,3])                                   */
int recmv_posenc_vjp(const float* x, int64_t ldx, const float* g, int64_t ldg, const float* t, int64_t ldt,
                     float* out, int64_t P, int L, const float* weights_host, void* stream);
int recmv_posenc_jvp(const float* x, int64_t ldx, const float* t, int64_t ldt, float* out, int64_t ldo, int64_t P,
                     int L, const float* weights_host, void* stream);

/* ------------------------------------------------------------------------------------------------
 * B2. SMPL kinematic chain of LBSkinner (model/Deformer.py:372-405; posedSkeleton :311-334), one kernel.
 *   poses [B,24,3] axis-angle -> G [B,24,4,4] (global joint transforms, `results`) and, when init_pose
 *   [24,4,4] and A are given, A = G . init_pose.  Js_host [24,3] and parents_host [24] are HOST arrays
 *   (constants of the skinner).  Backward: (gG, gA; either may be NULL) -> gposes [B,24,3].
 * ---------------------------------------------------------------------------------------------- */
int recmv_kinematic_chain_forward(const float* poses, const float* Js_host, const int32_t* parents_host,
                                  const float* init_pose, float* G, float* A, int64_t B, void* stream);
int recmv_kinematic_chain_backward(const float* poses, const float* Js_host, const int32_t* parents_host,
                                   const float* init_pose, const float* gG, const float* gA, float* gposes,
                                   int64_t B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-MLP launch chains (csrc/mlp_chain.hip): ONE call enqueues every kernel of a graph-free pass through
 * an MLP of the hot path — SDF net (model/network.py:98-133), offset MLP of the deformer
 * (model/Deformer.py:141-206) — on the caller's stream.  Used by the surface root finder
 * (utils/FindSurfacePs.py:273-353) and the no-grad grid queries of Seg3dLossless.
 *
 *   input   = [ gamma_L(x) | cond[cond_index[p]] ]                       (dims[0] = 3+6L+cond_dim)
 *   layer l = hidden_act(h W[l]^T + bias[l]);  W[l] is [rows[l], dims[l]] row-major
 *   layer l+1 == skip_layer: its input is [ layer l output | gamma_L(x) ] / sqrt(2)   (network.py:105-106)
 *   last layer: no activation; only its first n_out rows are evaluated; residual: out = x + out (Deformer.py:201-206)
 * Wt[l] = W[l]^T ([dims[l], rows[l]] row-major) is only read by recmv_mlp_vjp_input.
 * pe_weights: the 2L annealing weights (utils/utils.py:40-46), ones when not annealed.
 * Every function that takes a recmv_mlp validates it first, in one way (csrc/mlp_desc.h): an inconsistent descriptor is
 * RECMV_ERR_ARG with the function's name in front of the message, and 0 from the *_bytes functions and recmv_mlp_rows_supported.
 * ---------------------------------------------------------------------------------------------- */
#define RECMV_MLP_MAX_LAYERS 12
typedef struct recmv_mlp {
  int32_t n_layers, multires, cond_dim, skip_layer /* -1: none */, hidden_act, residual;
  float act_param;
  int32_t dims[RECMV_MLP_MAX_LAYERS + 1];
  int32_t rows[RECMV_MLP_MAX_LAYERS];
  const float* W[RECMV_MLP_MAX_LAYERS];
  const float* Wt[RECMV_MLP_MAX_LAYERS];
  const float* bias[RECMV_MLP_MAX_LAYERS];
  float pe_weights[32];
  /* optional second net of the same shape (ABI v5): rows [split_row, P) of a call use W2 / Wt2 / bias2 — the rows of two garments'
   * SDF nets evaluated as one block (recmv_gemm_nt_seg).  split_row = 0 or W2[0] == NULL: one net.  A multiple of 128. */
  const float* W2[RECMV_MLP_MAX_LAYERS];
  const float* Wt2[RECMV_MLP_MAX_LAYERS];
  const float* bias2[RECMV_MLP_MAX_LAYERS];
  int64_t split_row;
} recmv_mlp;

/* keep = 1 lays every layer's activation out separately (needed by recmv_mlp_vjp_input); keep = 0 ping-pongs. */
int64_t recmv_mlp_workspace_bytes(const recmv_mlp* m, int64_t P, int keep);
/* x [P,3]; cond [*, cond_dim] with row stride ld_cond, cond_index [P] (NULL: row 0 for every point); out [P,n_out]. */
int recmv_mlp_forward(const recmv_mlp* m, const float* x, const float* cond, int64_t ld_cond,
                      const int64_t* cond_index, int64_t P, int n_out, float* out, int64_t ldo,
                      void* workspace, int64_t workspace_bytes, int keep, void* stream);
/* gx [P,3] = J(x)^T g_out after recmv_mlp_forward(keep=1) on the same workspace.  g_out [P,n_out] (row stride
 * ldg), or NULL = ones with n_out == 1 (gradient of the scalar output). */
int recmv_mlp_vjp_input(const recmv_mlp* m, const float* x, int64_t P, int n_out, const float* g_out, int64_t ldg,
                        float* gx, void* workspace, int64_t workspace_bytes, void* stream);

/* Row-tile-persistent form of the two passes above for the few-thousand-row launches of the ray path (csrc/mlp_rows.hip): ONE
 * launch per pass — a workgroup keeps the activations of 16 rays in LDS across all layers (positional encoding, per-frame code
 * gather, skip concatenation, bias, activation, residual; in the reverse pass the activation gradients and the encoding's VJP),
 * the weights stream from L2 in MFMA-fragment order.  Replaces, like the chains, model/network.py:98-133 (SDF value + input
 * gradient) and model/Deformer.py:141-206 (offset MLP + VJP) as they are called by utils/FindSurfacePs.py:273-353.
 *   recmv_mlp_rows_supported : 1 when the descriptor fits (2..12 layers, every layer's inputs and outputs <= 512 wide — the last
 *                              layer's rows included, although only 16 of them can be evaluated —, <= 8 encoding bands, one net,
 *                              the skip connection not on layer 0); 0 otherwise: recmv_mlp_pack_bytes is then 0 and the pack and
 *                              the two passes return RECMV_ERR_ARG without a launch.
 *   recmv_mlp_pack(_bytes)   : lays every layer's weight (and its transpose) out in fragment order, zero-padded — once per
 *                              weight version; the packed buffer is what the two passes read.
 *   recmv_mlp_rows_forward   : as recmv_mlp_forward with n_out <= 16; keep = 1 stores the hidden activations in `workspace`
 *                              (recmv_mlp_rows_workspace_bytes) for the reverse pass.
 *   recmv_mlp_rows_vjp_input : as recmv_mlp_vjp_input, after recmv_mlp_rows_forward(keep = 1) on the same workspace.
 * Same arithmetic as the per-layer kernels (exact f32 MFMA products, f32 accumulation) in another summation order: results agree
 * to rounding.  Rows are independent of the tile they sit in.
 *   recmv_set_mlp_rows_tile  : rows per workgroup of the two passes — 1: 16 rows (one round of workgroups up to 4 096 rows: lowest
 *                              latency), 2: 32 rows (every weight byte from L2 feeds twice the FLOP, half the CUs per pass),
 *                              0 (default): 16 up to 4 096 rows, 32 above.  Process-global, like recmv_set_gemm_mode. */
int recmv_mlp_rows_supported(const recmv_mlp* m);
int recmv_set_mlp_rows_tile(int row_tiles);
int64_t recmv_mlp_pack_bytes(const recmv_mlp* m);
int recmv_mlp_pack(const recmv_mlp* m, void* packed, int64_t packed_bytes, void* stream);
int64_t recmv_mlp_rows_workspace_bytes(const recmv_mlp* m, int64_t P);
int recmv_mlp_rows_forward(const recmv_mlp* m, const void* packed, const float* x, const float* cond, int64_t ld_cond,
                           const int64_t* cond_index, int64_t P, int n_out, float* out, int64_t ldo, void* workspace,
                           int64_t workspace_bytes, int keep, void* stream);
int recmv_mlp_rows_vjp_input(const recmv_mlp* m, const void* packed, const float* x, int64_t P, int n_out, const float* g_out,
                             int64_t ldg, float* gx, const void* workspace, int64_t workspace_bytes, void* stream);

/* Strided element-wise helpers of the chains:
 *   recmv_act_grad_2d   : out[r,c] = out_scale * gy[r,c] * act'(z),  y = act(z) = y_scale * ybuf[r,c]; ldg may be 0
 *   recmv_add_scaled_2d : out[r,c] = a[r,c] + s * b[r,c]                                                       */
int recmv_act_grad_2d(const float* gy, int64_t ldg, const float* y, int64_t ldy, float* out, int64_t ldo,
                      int64_t rows, int64_t cols, int act, float act_param, float y_scale, float out_scale,
                      void* stream);
int recmv_add_scaled_2d(const float* a, int64_t lda, const float* b, int64_t ldb, float s, float* out, int64_t ldo,
                        int64_t rows, int64_t cols, void* stream);

/* ------------------------------------------------------------------------------------------------
 * First-hit mesh rasteriser (csrc/rasterize_meshes.hip).
 *   replaces `self.maskRender(def_garment_mesh)` -> Fragments in find_surface_ps
 *   (engineer/networks/OptimGarmentNetwork.py:742-767; settings :2336-2347) = pytorch3d 0.4.0
 *   `rasterize_meshes(faces_per_pixel=1, perspective_correct, clip_barycentric_coords=False)`, whose outputs feed
 *   utils/FindSurfacePs.py:7-37.
 * face_verts [total_faces,3,3] f32: NDC x, y (+x left, +y up; pixel column c is centred at x = 1-(2c+1)/W, row r at
 * y = 1-(2r+1)/H — model/CameraMine.py:132-142) and view-space depth z of the three corners of every face, meshes
 * packed one after another; mesh n owns faces [mesh_first_face[n], +mesh_num_faces[n]) (device int64 [N]);
 * max_faces_per_mesh >= max(mesh_num_faces) (host value, sizes the launch).  blur_radius is pytorch3d's (squared NDC
 * distance; 0 = hard coverage).  Outputs per pixel [N,H,W]: pix_to_face (packed face index, -1 = none), zbuf,
 * bary_coords [N,H,W,3], dists (signed squared distance to the nearest edge, negative inside); -1 where empty.
 * Ties in depth go to the lowest face index; the result does not depend on scheduling.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_rasterize_meshes_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t total_faces);
int recmv_rasterize_meshes(const float* face_verts, const int64_t* mesh_first_face, const int64_t* mesh_num_faces,
                           int64_t N, int64_t total_faces, int64_t max_faces_per_mesh, int64_t H, int64_t W,
                           float blur_radius, int perspective_correct, int cull_backfaces, int64_t* pix_to_face,
                           float* zbuf, float* bary_coords, float* dists, void* workspace, int64_t workspace_bytes,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * Vertex normals + hard Phong shading of rasterised meshes (csrc/shade_meshes.hip, ABI v10).
 *   replaces pytorch3d 0.4.0's `Meshes.verts_normals_packed` and `HardPhongShader` (phong_shading, PointLights,
 *   Materials, hard_rgb_blend) of the inference renders (engineer/networks/OptimGarmentNetwork.py:3216-3306, shader
 *   set by infer_fl.py), with the IoU mask error of :3241-3243 as optional integer counts.
 * recmv_verts_normals: verts [N,V,3] f32, ONE face table faces [F,3] int64 shared by the N meshes, the vertex -> (face,
 *   corner) adjacency adj_offsets [V+1] / adj_codes [3F] int32 (code = face * 3 + corner, each vertex's list ordered
 *   corner 1, corner 2, corner 0 and by ascending face inside each: pytorch3d's summation order) -> normals [N,V,3]
 *   = normalize(sum of corner cross products, eps 1e-6).  No float atomics: bitwise reproducible, independent of N.
 * recmv_hard_phong_shade: one thread per pixel.  pix_to_face [N,H,W] int64 packed (mesh * F + face, < 0 = empty) and
 *   bary_coords [N,H,W,3] of recmv_rasterize_meshes; colors [colors_batch,V,3] with colors_batch 1 or N (TexturesVertex);
 *   cam_centers [N,3] (camera centre per image, device); params_host: recmv_hard_phong_params_floats() host floats =
 *   light location[3], light ambient[3], diffuse[3], specular[3] colours, material ambient[3], diffuse[3], specular[3],
 *   shininess, background colour[3].  images [N,H,W,4] f32 RGBA (16-byte aligned): (ambient + diffuse) * texel +
 *   specular, background colour where empty, alpha 1.  gt_mask [N,H,W] f32 (nonzero = inside) and counts [N,2] int64
 *   (both or neither): counts[n] = (|M n G|, |M u G|) with M = (pix_to_face >= 0), exact and order independent.
 * ---------------------------------------------------------------------------------------------- */
int recmv_verts_normals(const float* verts, const int64_t* faces, const int32_t* adj_offsets, const int32_t* adj_codes,
                        int64_t N, int64_t V, int64_t F, float* normals, void* stream);
int64_t recmv_hard_phong_params_floats(void);
int recmv_hard_phong_shade(const int64_t* pix_to_face, const float* bary_coords, const float* verts, const float* normals,
                           const float* colors, int64_t colors_batch, const int64_t* faces, const float* cam_centers,
                           int64_t N, int64_t V, int64_t F, int64_t H, int64_t W, const float* params_host, float* images,
                           const float* gt_mask, int64_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Point-cloud rasteriser + alpha compositor, forward and backward (csrc/rasterize_points.hip).
 *   replaces `self.pcRender(Pointclouds(...))` of the mask loss (engineer/networks/OptimGarmentNetwork.py:937;
 *   PointsRendererWithFrags(_Split) model/CameraMine.py:306-415; settings engineer/networks/OptimNetwork.py:87-100:
 *   points_per_pixel = 50, radius 0.006 / 0.00465 / 0.0041) = pytorch3d 0.4.0 `rasterize_points` +
 *   `alpha_composite` and their backward passes.
 * points [total_points,3] f32: NDC x, y (same pixel convention as recmv_rasterize_meshes) and view depth z, clouds
 * packed one after another; cloud n owns points [cloud_first_point[n], +cloud_num_points[n]) (device int64 [N]).
 * Fragments, all [N,H,W,K] with K = points_per_pixel, K fastest: idx (packed point index, int32, -1 = none), zbuf,
 * dists (squared NDC distance of the point to the pixel centre; a point is listed when it is < radius^2 and z >= 0),
 * the K nearest in depth, sorted by (depth, index), packed to the front.
 *   recmv_rasterize_points_backward : grad_points [total_points,3] = d/dpoints of (grad_dists . dists + grad_zbuf . zbuf)
 *                                     (grad_zbuf may be NULL).  One thread per point sums its pixels in row-major order:
 *                                     deterministic (upstream accumulates with float atomics).
 *   recmv_alpha_composite_forward   : images [N,C,H,W]; images[n,c,y,x] = sum_k a_k prod_{l<k}(1 - a_l) features[c,idx_k]
 *                                     with alphas [N,H,W,K] and features [C,total_points].  radius2 == 0: `alphas`
 *                                     are the opacities.  radius2 != 0: `alphas` holds the rasteriser's dists and
 *                                     a = 1 - dists / radius2 (PointsRendererWithFrags' 1 - d2/radius^2,
 *                                     model/CameraMine.py:361-362, fused).  idx lists must be packed to the front.
 *   recmv_alpha_composite_backward  : grad_alphas [N,H,W,K] = gradient w.r.t. the `alphas` INPUT (opacities or
 *                                     dists), no atomics; grad_features [C,total_points] or NULL.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_rasterize_points_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t total_points, float radius);
int recmv_rasterize_points(const float* points, const int64_t* cloud_first_point, const int64_t* cloud_num_points,
                           int64_t N, int64_t total_points, int64_t max_points_per_cloud, int64_t H, int64_t W,
                           float radius, int points_per_pixel, int32_t* idx, float* zbuf, float* dists,
                           void* workspace, int64_t workspace_bytes, void* stream);
int recmv_rasterize_points_backward(const float* points, const int64_t* cloud_first_point,
                                    const int64_t* cloud_num_points, const int32_t* idx, const float* grad_dists,
                                    const float* grad_zbuf, int64_t N, int64_t total_points,
                                    int64_t max_points_per_cloud, int64_t H, int64_t W, float radius,
                                    int points_per_pixel, float* grad_points, void* stream);
int recmv_alpha_composite_forward(const int32_t* idx, const float* alphas, const float* features, int64_t N,
                                  int64_t H, int64_t W, int points_per_pixel, int64_t C, int64_t total_points,
                                  float radius2, float* images, void* stream);
int recmv_alpha_composite_backward(const int32_t* idx, const float* alphas, const float* features,
                                   const float* grad_images, int64_t N, int64_t H, int64_t W, int points_per_pixel,
                                   int64_t C, int64_t total_points, float radius2, float* grad_alphas,
                                   float* grad_features, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused linear-blend skinning on ray points and the root finder's per-ray step (csrc/lbs_fused.hip).
 *   replaces LBSkinner.forward with batch_inds (model/Deformer.py:405-445) and its input gradient, and the
 *   energy / update arithmetic of OptimizeGarmentSurfacePs (utils/FindSurfacePs.py:316-351), no autograd.
 * grid: the skinning-weight volume, CHANNELS-LAST [D,H,W,24] f32 (the memory of a torch channels_last_3d
 * [1,24,D,H,W] tensor), sampled trilinearly at (p - center) * scale (scale = 2 / bbox extent) with the
 * GridSamplerMine semantics (border padding, align_corners=False).
 *   recmv_lbs_forward   : d = (sum_j w_j A[frame,j]) [p;1] + trans[frame];  A [B,24,4,4], trans [B,3].
 *                         With rays [P,3] and cam [3] (device): loss2 = |(d-c) x v| / |d-c|, angle (degrees) and
 *                         g_d = d loss2 / d d.  rays == NULL skips those outputs.
 *   recmv_lbs_vjp_input : g_p [P,3] = J_d(p)^T g_d.
 *   recmv_rootfind_update: unfinished &= !(|f| < dthreshold && angle < athreshold); on unfinished rays (and
 *                         do_update != 0) p -= E grad / |grad|^2 with E = w1|f| + w2 loss2,
 *                         grad = w1 sign(f) gf + w2 gd; *counter += number of unfinished rays.
 * B (frames) is 1..128.  The entry points that take A stage its rows 0..2 in dynamic LDS, B * 24 * 12 * 4 bytes: 147 456 bytes
 * at B = 128.  What one launch may ask for is a property of the device, not a constant of the HIP headers
 * (hipDeviceAttributeMaxSharedMemoryPerBlock, hip_runtime_api.h); gfx950 reports 163 840 bytes (the CU's 160 KiB) for it and for
 * hipDeviceAttributeSharedMemPerBlockOptin, so B = 128 fits and is an ordinary case of tests/test_gpu_skinning.py.
 * ---------------------------------------------------------------------------------------------- */
typedef struct recmv_lbs_grid {
  const float* volume;
  int64_t D, H, W;
  float center[3];
  float scale[3];
} recmv_lbs_grid;

int recmv_lbs_forward(const float* ps, const int64_t* frame, int64_t P, const float* A, const float* trans,
                      int64_t B, const recmv_lbs_grid* grid, const float* cam, const float* rays, float* d,
                      float* loss2, float* angle, float* g_d, void* stream);
int recmv_lbs_vjp_input(const float* ps, const int64_t* frame, int64_t P, const float* A, int64_t B,
                        const recmv_lbs_grid* grid, const float* g_d, float* g_p, void* stream);
/* Parameter side of the skinning VJP, staged for two fixed-order reductions: W [P,24] (sampled blend weights),
 * Q [P, B*12] = g_d (x) [p;1] in the point's frame block (zeros elsewhere), Gs [P, B*3] = g_d likewise.  Then
 * gA[b,j,i,k] = recmv_gemm_tn(W, Q)[j, b*12 + 4i + k] and gtrans[b,i] = recmv_colsum(Gs)[b*3 + i]. */
int recmv_lbs_vjp_params_stage(const float* ps, const int64_t* frame, int64_t P, int64_t B,
                               const recmv_lbs_grid* grid, const float* g_d, float* W, float* Q, float* Gs,
                               void* stream);
/* The skinning stage as a jet (ABI v9): v [P,3] as recmv_lbs_forward and J [P,9] = d v / d p (row i = gradient of v_i) in one
 * launch — replaces LBSkinner.forward + the three create_graph autograd.grad calls of utils/utils.py:133-156 (compute_Jacobian) at
 * the converged ray points — and its first-order reverse: g_p [P,3] per point, the parameter side staged as W4 [4P,24],
 * Q4 [4P, B*12], Gs [P, B*3] for gA[b,j,i,k] = recmv_gemm_tn(W4, Q4)[j, b*12 + 4i + k], gtrans = recmv_colsum(Gs).  gv / gJ: the
 * cotangents of v and J, either may be NULL (zeros). */
int recmv_lbs_jet_forward(const float* ps, const int64_t* frame, int64_t P, const float* A, const float* trans,
                          int64_t B, const recmv_lbs_grid* grid, float* v, float* J, void* stream);
int recmv_lbs_jet_backward_stage(const float* ps, const int64_t* frame, int64_t P, const float* A, int64_t B,
                                 const recmv_lbs_grid* grid, const float* gv, const float* gJ, float* g_p, float* W4,
                                 float* Q4, float* Gs, void* stream);
int recmv_rootfind_update(float* p, const float* f, const float* gf, const float* loss2, const float* angle,
                          const float* gd, uint8_t* unfinished, int32_t* counter, int64_t P, float dthreshold,
                          float athreshold, float w1, float w2, int do_update, void* stream);
/* The same step with the step index on the device, so that all steps of an iteration are one and the same launch (a
 * step captured in a hipGraph can be replayed).  counters / marks: int32 [times + 2], zero-initialised by the caller;
 * state: int32 [1] = index of the step to run (0 at the start).  Runs the update with do_update = (step < times),
 * counters[step] += unfinished rays; then marks[step] = counters[step] + 1 and state[0] = step + 1.  A host that polls an
 * asynchronous copy of `marks` reads 0 for "not run yet" and 1 for "no unfinished ray" (utils/FindSurfacePs.py:311-313). */
int recmv_rootfind_step(float* p, const float* f, const float* gf, const float* loss2, const float* angle,
                        const float* gd, uint8_t* unfinished, int32_t* counters, int32_t* marks, int32_t* state,
                        int64_t P, float dthreshold, float athreshold, float w1, float w2, int times, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of one fused layer y = act(x W^T + b) in one call (csrc/linear_bwd.hip) — autograd of nn.Linear +
 * activation in the reference (model/network.py:98-111 etc.).  y, gy [M,N]; x [M,K]; Wt = W^T [K,N];
 * outputs gx [M,K] = (gy . act') W, gW [N,K] = (gy . act')^T x, gb [N] = column sums; any output may be NULL.
 * M = 0 (an empty batch): gW and gb are zeroed, gx is empty; gy, y, x, Wt and the workspace are neither read nor checked (may be NULL).
 * recmv_colsum: out[c] = sum_r g[r*ld + c], fixed summation order (deterministic).
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_colsum_workspace_bytes(int64_t rows, int64_t cols);
int recmv_colsum(const float* g, int64_t ld, int64_t rows, int64_t cols, float* out, void* workspace,
                 int64_t workspace_bytes, void* stream);
int64_t recmv_linear_backward_workspace_bytes(int64_t M, int64_t N, int64_t K);
int recmv_linear_backward(const float* gy, int64_t ldgy, const float* y, int64_t ldy, const float* x, int64_t ldx,
                          const float* Wt, int64_t ldwt, int64_t M, int64_t N, int64_t K, int act, float act_param,
                          float* gx, int64_t ldgx, float* gW, float* gb, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * MLP "jet" pass (csrc/mlp_jet.hip): value and input-Jacobian in one forward sweep (three tangent rows per point
 * carried through the layers), with an explicit first-order reverse sweep.  Replaces autograd's double backward for
 * the terms of the loss that differentiate grad_x SDF (model/network.py:121-133, OptimGarmentNetwork.py:1108-1119,
 * :1169-1172) and the Jacobian of the offset MLP (utils/utils.py:133-156, OptimGarmentNetwork.py:1135-1155).
 *   forward : y [P, rows_last] (residual nets: x + mlp), tang [3P, n_j] with tang[k*P + p, j] = d y_j / d x_k of the
 *             MLP part (the residual's identity is NOT included).
 *   backward: cotangents gy [P, rows_last] / gtang [3P, n_j] (NULL = zeros) -> gW[l] [rows[l], dims[l]], gb[l],
 *             g_in [4P, pad4(dims[0])] (cotangent of the stacked layer-0 input; rows [0,P) x columns [3+6L, dims[0])
 *             are the per-point cotangents of the gathered code) and gx [P,3]; each may be NULL.
 * eye3: 9 floats on the device = the 3x3 identity.  The workspace carries the activations from forward to backward.
 * One net: a descriptor that carries a second weight set (split_row > 0 and W2[0]) is RECMV_ERR_ARG in both passes.
 * recmv_gather_rows: out[r, 0:cols] = table[index[r] (or 0), 0:cols], columns [cols, fill) zeroed.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_mlp_jet_workspace_bytes(const recmv_mlp* m, int64_t P);
int recmv_mlp_jet_forward(const recmv_mlp* m, const float* x, const float* cond, int64_t ld_cond,
                          const int64_t* cond_index, const float* eye3, int64_t P, int n_j, float* y, int64_t ldy,
                          float* tang, void* workspace, int64_t workspace_bytes, void* stream);
int recmv_mlp_jet_backward(const recmv_mlp* m, const float* x, const float* eye3, int64_t P, int n_j, const float* gy,
                           int64_t ldgy, const float* gtang, float* const* gW, float* const* gb, float* g_in,
                           float* gx, void* workspace, int64_t workspace_bytes, void* stream);
int recmv_gather_rows(const float* table, int64_t ldt, const int64_t* index, float* out, int64_t ldo, int64_t rows,
                      int64_t cols, int64_t fill, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-launch HIP-event timing of the MFMA kernels, for the bench's roofline object.  Between
 * recmv_profile_begin() and recmv_profile_end() every gemm_nt / gemm_tn launch (from Python or from inside the
 * launch chains) is bracketed by events recorded on its launch stream.  recmv_profile_end fills, per kernel variant
 * v (0..7: gemm_nt_kernel<T, FAST, AMUL>, v = (T-1) + 2*FAST + 4*AMUL; 8: gemm_tn_occ_kernel / gemm_tn_kernel, the product
 * alone without its split-K reduction pass; 9 / 10: gemm_nt_occ_kernel<false, ...> with 128x128 / 64x128 tiles; 11:
 * gemm_nt_occ_kernel<true, ...>;
 * 12 / 13: gemm_nt_narrow_kernel<true, false, .> / its other instantiations — a caller that passes fewer than 14 slots gets
 * 9..13 folded into 3 / 3 / 7 / 2 / 6, the slots that carried those launches before):
 * out[5v] = timed launches, out[5v+1] = their summed duration [s], out[5v+2] = their summed algorithmic FLOP
 * (2 M N K), out[5v+3] / out[5v+4] = launches / FLOP of the launches smaller than `min_flops`, which are counted
 * but not bracketed (out must hold 5 * n_variants doubles, n_variants >= 9).
 * ---------------------------------------------------------------------------------------------- */
int recmv_profile_begin(double min_flops);
int recmv_profile_end(double* out, int n_variants);
/* Algorithmic bytes, 4 (M K + N K + M N), of the launches the last recmv_profile_end bracketed, per variant (same slots as its `out`:
 * out[v]).  With their summed duration this is the kernel's HBM-side roofline beside its MFMA one.  (ABI v7) */
int recmv_profile_bytes(double* out, int n_variants);
/* The launches of >= 4 GFLOP among the bracketed ones: out[3v] launches, out[3v+1] seconds, out[3v+2] FLOP.  (ABI v7) */
int recmv_profile_large(double* out, int n_variants);
/* After recmv_profile_end: out2[0] = seconds in which at least ONE bracketed launch was running (union of the event intervals of all
 * streams on one time axis), out2[1] = seconds from the first bracketed start to the last bracketed end. */
int recmv_profile_busy(double* out2);

/* ------------------------------------------------------------------------------------------------
 * Non-rigid ICP of a garment template (csrc/nricp.hip; added to ABI v10, no existing signature changed).  No float
 * atomics: bitwise reproducible.
 * recmv_knn1: exact 1-nearest neighbour of every source point p [N,3] f32 among the targets q [M,3] f32 (pytorch3d
 *   knn_points K=1): idx [N] int64 and squared distance dist [N] f32; ties go to the lowest target index.  N = 0 is a
 *   no-op, M = 0 an argument error.  Workspace: recmv_knn1_workspace_bytes(N), 8-byte aligned.
 * recmv_nricp_energy: one inner iteration of NRICP_Optimizer_AdamW at the affine maps A [N,3,3], b [N,3] of the rest
 *   positions x [N,3], closest points c [N,3] with normals nc [N,3], template normals nx [N,3], interior [N] u8;
 *   edges [E,2] int64 (unique undirected), inc_offsets [N+1] / inc_edges [2E] int32 (vertex -> incident edges),
 *   nbr_offsets [N+1] / nbr_idx [2E] int32 (vertex -> neighbours, degree = row length).  Writes scalars [4] f32 =
 *   (loss, vert_sum, stiff_sum, lap) on the device, the weight mask [N] u8 and the gradients dA [N,3,3], db [N,3].
 *   Workspace: recmv_nricp_energy_workspace_bytes(N), 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_knn1_workspace_bytes(int64_t N);
int recmv_knn1(const float* p, int64_t N, const float* q, int64_t M, int64_t* idx, float* dist, void* workspace,
               int64_t workspace_bytes, void* stream);
int64_t recmv_nricp_energy_workspace_bytes(int64_t N);
int recmv_nricp_energy(const float* A, const float* b, const float* x, const float* c, const float* nc, const float* nx,
                       const uint8_t* interior, const int64_t* edges, int64_t E, const int32_t* inc_offsets,
                       const int32_t* inc_edges, const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t N,
                       float gamma, float stiffness_weight, float laplacian_weight, float threshold, float* scalars,
                       uint8_t* mask, float* dA, float* db, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Laplacian alignment of a garment template to its feature curves (csrc/lap_align.hip; added to ABI v10, no existing
 * signature changed).  No float atomics: bitwise reproducible.  The neighbour CSR is nricp.neighbours_csr's:
 * nbr_offsets [V+1] / nbr_idx [nnz] int32, symmetric, degree = row length.
 * recmv_lap_align_solve: u [V,3] f32 = the solution of (L^T L + diag(cw)) u = L^T (L v) + cwt for the three columns, L the
 *   uniform Laplacian of pytorch3d's laplacian_packed, v [V,3] f32, cw [V] f64 (weight x constraints on the vertex), cwt
 *   [V,3] f64 (weight x sum of their targets).  Jacobi-preconditioned CG in f64 from u = v until |r| <= tol |rhs| in every
 *   column or max_iter iterations; a column freezes (alpha = beta = 0) when it converges or when p.q is not > 0 or
 *   alpha / beta is not finite.  The call synchronises `stream` once every 32 iterations and at the end.
 *   iterations (host, 1 int32) and residuals (host, 3 doubles: each column's final relative residual) are written on
 *   return.  V = 0 is a no-op.  Workspace: recmv_lap_align_workspace_bytes(V), 256-byte aligned.
 * recmv_lap_smooth: out [V,3] f32 = (1/deg_i) sum_{j in N(i)} u_j, accumulated in f64 in CSR order and rounded once; an
 *   isolated vertex -> 0.  out must not alias u.  V = 0 is a no-op.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_lap_align_workspace_bytes(int64_t V);
int recmv_lap_align_solve(const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t V, int64_t nnz, const float* v,
                          const double* cw, const double* cwt, double tol, int32_t max_iter, float* u, int32_t* iterations,
                          double* residuals, void* workspace, int64_t workspace_bytes, void* stream);
int recmv_lap_smooth(const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t V, int64_t nnz, const float* u, float* out,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Isotropic remeshing and Loop subdivision of a garment template (csrc/iso_remesh.hip; added to ABI v10, no existing
 * signature changed).  They replace pymeshlab's meshing_isotropic_explicit_remeshing / meshing_surface_subdivision_loop,
 * which the reference calls between its two NR-ICP passes.  No float atomics: bitwise reproducible.  The neighbour CSR is
 * nricp.neighbours_csr's: nbr_offsets [V+1] / nbr_idx [nnz] int32, symmetric, ascending per row.
 * recmv_closest_point: the exact closest point on the triangle mesh verts [V,3] f32 / faces [F,3] int64 of every query
 *   point p [P,3] f32 (Ericson's point-triangle test in f32, brute force over the faces): face [P] int64, point [P,3] f32
 *   and squared distance dist2 [P] f32; ties go to the lowest face id, a face with an index outside [0, V) is skipped.
 *   P = 0 is a no-op, V = 0 or F = 0 an argument error.  Workspace: recmv_closest_point_workspace_bytes(P), 8-byte aligned.
 * recmv_iso_relax: out [V,3] f32 = p + (I - n n^T)(c - p) for every vertex with fixed[i] == 0 and at least one neighbour,
 *   c the mean of its neighbours (f64, CSR order) and n = normals [V,3] (unit); other vertices are copied.  out must not
 *   alias verts.  V = 0 is a no-op.
 * recmv_loop_subdivide: Loop's scheme into out [V+E,3] f32.  Rows 0..V-1 (even): a vertex with boundary_nbrs [V,2]
 *   int64 >= 0 gets 3/4 p + 1/8 (b0 + b1), any other (1 - n beta) p + beta sum of its n neighbours, beta = (5/8 - (3/8 +
 *   1/4 cos(2 pi / n))^2) / n.  Row V + e (odd): edge_table [E,4] int64 = (a, b, c, d) gives 3/8 (a + b) + 1/8 (c + d), or
 *   1/2 (a + b) when d = -1 (a boundary edge).  out must not alias verts.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_closest_point_workspace_bytes(int64_t P);
int recmv_closest_point(const float* p, int64_t P, const float* verts, int64_t V, const int64_t* faces, int64_t F,
                        int64_t* face, float* point, float* dist2, void* workspace, int64_t workspace_bytes, void* stream);
int recmv_iso_relax(const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t V, int64_t nnz, const float* verts,
                    const float* normals, const uint8_t* fixed, float* out, void* stream);
int recmv_loop_subdivide(const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t V, int64_t nnz, const float* verts,
                         const int64_t* boundary_nbrs, const int64_t* edge_table, int64_t E, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Body-collision repair of posed garment meshes (csrc/mesh_collide.hip; added to ABI v10, no existing signature changed).
 * Not in the reference: the animation on novel poses (infer_fl_animation.py --fix-collisions) pushes garment vertices
 * that sank into the posed body back out.  No float atomics: bitwise reproducible.  B frames, one face table faces [F,3]
 * int64 for all of them (a face with an index outside [0, V) is skipped), body verts [B,V,3] f32.
 * recmv_point_mesh_nearest: for every point p [B,N,3] f32 the exact nearest triangle of its frame's body mesh (Ericson's
 *   point-triangle test in f32, brute force over the faces): face [B,N] int64 (-1: none) and squared distance sqdist
 *   [B,N] f32; ties go to the lowest face id.  B = 0 or N = 0 is a no-op, V = 0 or F = 0 an argument error.  Workspace:
 *   recmv_point_mesh_nearest_workspace_bytes(B, N), 8-byte aligned.
 * recmv_collision_push: with face [B,N] of recmv_point_mesh_nearest and the unit vertex normals vnormals [B,V,3]
 *   (recmv_verts_normals): q = closest point of p on its face with barycentric weights w, n = normalize(sum_i w_i
 *   vnormal_i), s = (p - q) . n.  s >= eps: p_out = p bit for bit; -max_depth <= s < eps: p_out = p + (eps - s) n and
 *   moved[b] += 1; s < -max_depth: p_out = p and unresolved[b] += 1 (a vertex that deep is nearer the far side of a limb).
 *   A vertex without a face or with a vanishing normal is copied.  moved / unresolved: int32 [B], zeroed by the call
 *   (integer atomics).  p_out may be p.  B = 0 is a no-op; N = 0 only zeroes the counts.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_point_mesh_nearest_workspace_bytes(int64_t B, int64_t N);
int recmv_point_mesh_nearest(const float* p, const float* verts, const int64_t* faces, int64_t B, int64_t N, int64_t V,
                             int64_t F, int64_t* face, float* sqdist, void* workspace, int64_t workspace_bytes,
                             void* stream);
int recmv_collision_push(const float* p, const float* verts, const float* vnormals, const int64_t* faces,
                         const int64_t* face, int64_t B, int64_t N, int64_t V, int64_t F, float eps, float max_depth,
                         float* p_out, int32_t* moved, int32_t* unresolved, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Feature-curve tubes (csrc/curve_tubes.hip; added to ABI v10, no existing signature changed):
 * `Intersect_Free_Curve.curve_to_mesh`, engineer/utils/garment_structure.py:176-274.
 * recmv_curve_tubes: closed curves [L,S,3] f32 with one normal each nx [L,3] f32 -> tubes of num_joints vertices per
 *   sample: verts [L,S*J,3] f32 (ring-major) and faces [L,2*S*J,3] int64 (indices local to the curve), one launch.
 *   Tangent d_i = (c_i - c_{i+1}) / (|.| + 1e-6) (the last one closes the curve); ring vertex c_i + radius (n cos t +
 *   (d x n) sin t + d * (d * n) (1 - cos t)), t = radians(j (360 / J)), the last product ELEMENTWISE as in the
 *   reference; faces (a_v, b_v, b_v+1), (a_v, b_v+1, a_v+1) for ring a, its successor b.  L, S or J below 1 and a J that
 *   does not divide 360 are argument errors.
 * recmv_curve_fit_step: value and gradient of the fit of the curves to polylines (:179-212).  The curves are x = center
 *   [L,1,3] + dirs [L,S,3] init_scale [L,S,1] relu(scale [L,S,1]) + nx_scale [L,S,1] nx [L,1,3]; pair p fits curve
 *   target_idx[p] (int32 [P], device) to the polyline targets[p] ([P,M,3] f32):
 *     loss[p] = w_cham (mean_i min_j |x_i - y_j|^2 + mean_j min_i |x_i - y_j|^2) + w_smooth sum_{k<S-1} (1 - cos(u_k, u_k+1))
 *   with the unit tangents u of the closed curve.  g_scale, g_nx_scale [L,S,1] f32 receive d(sum_p loss[p]) / d(scale,
 *   nx_scale) (zero for a curve no pair targets; pairs of one curve add in pair order).  A pair whose index is outside
 *   [0, L) gets loss 0.  One workgroup per curve with both point sets in LDS: (12 S + 4 M) * 4 bytes must fit 64 KiB - 64.
 *   No float atomics, fixed summation order: bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */
int recmv_curve_tubes(const float* curves, const float* nx, float radius, int64_t L, int64_t S, int64_t num_joints,
                      float* verts, int64_t* faces, void* stream);
int recmv_curve_fit_step(const float* center, const float* dirs, const float* init_scale, const float* nx,
                         const float* scale, const float* nx_scale, const float* targets, const int32_t* target_idx,
                         int64_t L, int64_t S, int64_t P, int64_t M, float w_cham, float w_smooth, float* loss,
                         float* g_scale, float* g_nx_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Uniform grid over a triangle mesh and the exact closest point through it (csrc/mesh_grid.hip).  Not in the reference: the
 * search of the evaluation metrics (recmv/metrics.py, eval_fl.py).  Integer atomics only.  One struct recmv_mesh_grid in HOST
 * memory describes a grid to the entry points below and to the queries of the next two sections (ABI v11):
 *   geometry: nx x ny x nz cubic cells of size cell_size with the corner at origin, chosen by the caller so that it covers
 *     the mesh; cell (x, y, z) has index (z ny + y) nx + x; at most 2^26 cells; a coordinate outside is clamped to the edge.
 *   tables (device): offsets [cells + 1] int32, entries [n_entries] int32 with n_entries < 2^31 — the face ids of cell c at
 *     offsets[c] .. offsets[c + 1] — and tris [F,12] f32, 16-byte aligned: every face as (a, b - a, c - a, 0, 0, 0).
 * Every entry point checks the geometry, n_entries and the tables it reads or writes before any HIP call, like its other
 * arguments (negative sizes, NULL pointers with non-zero sizes); a NULL descriptor is an argument error.
 * recmv_mesh_grid_count [reads the geometry]: counts [cells] int32 = the faces of verts [V,3] f32 / faces [F,3] int64 whose
 *   axis-aligned box overlaps each cell (conservative; a face with an index outside [0, V) is binned nowhere), total [1] int64
 *   (device, 8-byte aligned) = their sum, the number of (cell, face) entries.  Both are zeroed by the call.
 * recmv_mesh_grid_fill [reads the geometry and n_entries, the CAPACITY of entries; writes through offsets, entries, tris]:
 *   offsets = the exclusive scan of counts (offsets[cells] the total, which must be below 2^31), entries in an order that
 *   depends on scheduling (a slot at or beyond the capacity is not written), tris.  The geometry of the count call.
 *   Workspace: recmv_mesh_grid_workspace_bytes(cells), 4-byte aligned.
 * recmv_closest_point_grid [reads the geometry and every table]: recmv_closest_point's outputs for the query points p [P,3]
 *   f32 — face [P] int64 (-1: none), point [P,3] f32, dist2 [P] f32, ties to the lowest face id, bit for bit what
 *   recmv_closest_point gives on the mesh of F faces the grid was built from — by visiting the Chebyshev rings of cells
 *   around the query's cell until everything outside them is farther than the best found.  order: NULL, or a permutation [P]
 *   int64 of the queries (thread t handles query order[t]: sorted by cell, neighbouring lanes read the same cells); lanes:
 *   1, 8 or 64 lanes of a wave per query.  P = 0 is a no-op, F = 0 an argument error.
 * ---------------------------------------------------------------------------------------------- */
typedef struct recmv_mesh_grid {
  float origin[3];
  float cell_size;
  int64_t nx, ny, nz;
  int32_t* offsets;
  int32_t* entries;
  int64_t n_entries;
  float* tris;
} recmv_mesh_grid;

int64_t recmv_mesh_grid_workspace_bytes(int64_t cells);
int recmv_mesh_grid_count(const float* verts, int64_t V, const int64_t* faces, int64_t F, const recmv_mesh_grid* grid,
                          int32_t* counts, int64_t* total, void* stream);
int recmv_mesh_grid_fill(const float* verts, int64_t V, const int64_t* faces, int64_t F, const recmv_mesh_grid* grid,
                         const int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);
int recmv_closest_point_grid(const float* p, int64_t P, const int64_t* order, int64_t F, const recmv_mesh_grid* grid,
                             int32_t lanes, int64_t* face, float* point, float* dist2, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Which faces of two triangle meshes cross (csrc/mesh_intersect.hip, csrc/tri_tri.h; added to ABI v10, no existing
 * signature changed).  Not in the reference.  Meshes as above: verts [V,3] f32, faces [F,3] int64.  A result is a pair
 * (i, j), face i of A and face j of B, whose closed boxes meet and that cross PROPERLY: one of the six edge-against-triangle
 * tests holds with every inequality strict, so touching (a shared vertex or edge, a vertex exactly in the other's plane),
 * coplanar overlap, a face without area and anything with a NaN are no crossing; a face with an index outside [0, V) crosses
 * nothing.  self_mode = 1: A and B are the same mesh (the same pointers and sizes), only i < j; skip_shared = 1 (self_mode
 * only, an argument error otherwise): a pair of faces that share a vertex index is skipped.  Integer atomics only.
 * Two passes.  Count pass: counts [FA] int32 = the pairs of each face of A, total [1] int64 (device, 8-byte aligned) = their
 *   sum; both zeroed by the call.  The caller scans counts into offsets [FA + 1] int32 (exclusive; offsets[FA] the total).
 *   Fill pass: pairs [capacity,2] int32 = the pairs of face i at offsets[i] .. offsets[i + 1], in an order that depends on
 *   scheduling; cursor [FA] int32 is workspace; dropped [1] int64 (device, 8-byte aligned) = the pairs found that had no
 *   slot below their face's end and below capacity (0 when the passes agree and capacity >= total) — they are not written.
 * recmv_mesh_intersect_brute: every pair of faces.  counts and total given, offsets NULL: the count pass; offsets given,
 *   counts NULL: the fill pass.
 * recmv_mesh_intersect_grid_count / _fill: through the grid built over B by recmv_mesh_grid_count / _fill (reads the
 *   descriptor's geometry, offsets, entries and n_entries; not tris): the same pairs as the brute force.  lanes: 1, 8 or 64
 *   lanes of a wave per face of A; it does not change the result.
 * Argument errors are found before any HIP call.  An empty A or B gives no pair (counts and total zeroed).
 * ---------------------------------------------------------------------------------------------- */
int recmv_mesh_intersect_brute(const float* a_verts, int64_t VA, const int64_t* a_faces, int64_t FA, const float* b_verts,
                               int64_t VB, const int64_t* b_faces, int64_t FB, int32_t self_mode, int32_t skip_shared,
                               int32_t* counts, int64_t* total, const int32_t* offsets, int32_t* pairs, int64_t capacity,
                               int32_t* cursor, int64_t* dropped, void* stream);
int recmv_mesh_intersect_grid_count(const float* a_verts, int64_t VA, const int64_t* a_faces, int64_t FA,
                                    const float* b_verts, int64_t VB, const int64_t* b_faces, int64_t FB,
                                    const recmv_mesh_grid* grid, int32_t lanes, int32_t self_mode, int32_t skip_shared,
                                    int32_t* counts, int64_t* total, void* stream);
int recmv_mesh_intersect_grid_fill(const float* a_verts, int64_t VA, const int64_t* a_faces, int64_t FA,
                                   const float* b_verts, int64_t VB, const int64_t* b_faces, int64_t FB,
                                   const recmv_mesh_grid* grid, int32_t lanes, int32_t self_mode, int32_t skip_shared,
                                   const int32_t* offsets, int32_t* pairs, int64_t capacity, int32_t* cursor,
                                   int64_t* dropped, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Segments against a triangle mesh (csrc/segment_mesh.hip, csrc/seg_tri.h; added to ABI v10, no existing signature
 * changed).  The reference casts rays with pyembree (engineer/optimizer/surface_intesection.py).  Segments p [S,3], q [S,3]
 * f32, the mesh as above.  Segment pq HITS face abc iff orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs and
 * orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) strictly the same sign (csrc/tri_tri.h's edge-against-triangle test), and
 * the segment passes the face's box (csrc/seg_tri.h's gate, implied by a hit in exact arithmetic).  Strict: touching (an
 * endpoint exactly in the plane, a segment through a vertex or along an edge), a segment in the face's plane, a face without
 * area, a segment whose endpoints are the same bits and anything not finite are no hit; a face with an index outside [0, V)
 * is hit by nothing.  t = sp / (sp - sq), sp = orient(a,b,c,p), sq = orient(a,b,c,q), kept within the parameters at which
 * the segment is within 40 eps32 S (S the largest |coordinate| of p and q) of the face's box (csrc/seg_tri.h's seg_clamp_t:
 * no change where the determinants mean something, and what lets the first-hit walk stop where they are noise).
 * Outputs: face [S] int64 = the hit with the smallest t, ties to the lowest face id (-1: none), t [S] f32 (NaN: none),
 *   count [S] int32 = the number of faces hit.  No atomics.  S = 0 is a no-op; F = 0 hits nothing.
 * recmv_segment_mesh_brute: every face.
 * recmv_segment_mesh_grid: through the grid built over the mesh by recmv_mesh_grid_count / _fill (reads the descriptor's
 *   geometry, offsets, entries and n_entries; not tris): bit for bit the brute force's outputs.  lanes: 1, 8 or 64 lanes of a
 *   wave per segment; it does not change the result.  want_count = 1: the whole segment is walked and count written;
 *   want_count = 0: the walk may stop behind the first hit, count is not written and may be NULL.
 * Argument errors (negative sizes, NULL pointers, lanes, dims below 1, a cell size that is not positive and finite,
 * want_count = 1 without count) are found before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
int recmv_segment_mesh_brute(const float* p, const float* q, int64_t S, const float* verts, int64_t V, const int64_t* faces,
                             int64_t F, int64_t* face, float* t, int32_t* count, void* stream);
int recmv_segment_mesh_grid(const float* p, const float* q, int64_t S, const float* verts, int64_t V, const int64_t* faces,
                            int64_t F, const recmv_mesh_grid* grid, int32_t lanes, int32_t want_count, int64_t* face, float* t,
                            int32_t* count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The sums of one ICP iteration (csrc/icp.hip; added to ABI v11, no existing signature changed).  The reference's
 * engineer/optimizer/icp_optimzier.py fits a rotation and a translation to nearest neighbours in torch; recmv/align.py
 * iterates a rigid or similarity fit of a mesh to a mesh and takes its normal equations from here.  No float atomics.
 * Inputs: x [P,3] f32, the source points under the current transform; q [P,3] f32, face [P] int64 and dist2 [P] f32 exactly
 *   as recmv_closest_point or recmv_closest_point_grid returned them for x on the mesh verts [V,3] f32 / faces [F,3] int64
 *   (q is taken as given, not recomputed); border [F] uint8 on the device or NULL; max_dist2 [1] f32 on the device or NULL;
 *   centre [3] float64 in HOST memory; with_plane 0 or 1.
 * Pair i is ACCEPTED iff all of: 0 <= face[i] < F and the face's three indices lie in [0, V); x_i, q_i and dist2[i] are
 *   finite; max_dist2 is NULL or dist2[i] <= *max_dist2 (equality accepted, a NaN threshold accepts nothing); border is NULL or
 *   the closest point does not lie on the border: csrc/closest_tri.h's point-triangle test of x_i against the face, as the
 *   search ran it, ends in an edge or vertex region, and the pair is rejected when that region's bit of border[face] is set —
 *   bit 0 / 1 / 2: edge ab / ac / bc is a border edge, bit 3 / 4 / 5: vertex a / b / c is a border vertex; and with
 *   with_plane = 1 the face normal (b - a) x (c - a) has a finite length that is not zero.
 * Output: sums [RECMV_ICP_SUMS] float64 on the device, over the accepted pairs, with c = centre, u = (double)x - c,
 *   w = (double)q - c, m the unit face normal formed in double from the f32 vertex coordinates, g = u x m,
 *   J = (g0, g1, g2, m0, m1, m2, u.m) and r = (u - w).m:
 *     [0] the count; [1..3] sum u; [4..6] sum w; [7 + 3a + b] sum u_a w_b; [16] sum |u|^2; [17] sum |w|^2; [18] sum |u - w|^2;
 *     [19..46] the upper triangle (row-major, j <= k) of sum J J^T; [47..53] sum J r; [54] sum r^2; [55] 0 (reserved).
 *   Entries 19 .. 55 are exact zeros with with_plane = 0.  Every successful call writes all of sums; P = 0 writes zeros.
 * Reproducible: threads take the pairs in a fixed pattern, waves meet in a fixed shuffle tree, a block's waves in wave order,
 *   and a second one-block launch adds the blocks' slabs in block order; the number of blocks depends on P alone, so the same
 *   input gives the same bits on every run and every card.
 * Workspace: recmv_icp_accumulate_workspace_bytes(P) (0 for P = 0), 8-byte aligned; too small or misaligned is
 *   RECMV_ERR_WORKSPACE.  Argument errors (negative sizes, NULL pointers with P > 0, V = 0 or F = 0 with P > 0, NULL centre or
 *   sums, with_plane outside {0, 1}) are found before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
#define RECMV_ICP_SUMS 56
int64_t recmv_icp_accumulate_workspace_bytes(int64_t P);
int recmv_icp_accumulate(const float* x, const float* q, const int64_t* face, const float* dist2, int64_t P,
                         const float* verts, int64_t V, const int64_t* faces, int64_t F, const uint8_t* border,
                         const float* max_dist2, const double* centre, int32_t with_plane, double* sums, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * What a mesh is made of (csrc/mesh_topology.hip; added to ABI v11, no existing signature changed).  Not in the reference.
 * The kernels of recmv/topology.py: connected components, per-face figures, reproducible per-segment sums.  Integer atomics
 * only.  Argument errors (negative sizes, K, C, NULL pointers with work to do, a workspace too small) are found before any
 * HIP call; an empty input is a no-op that returns RECMV_OK.
 * recmv_graph_components: a graph of n nodes and links [M,K] int64, K = 2 or 3; a row joins its K nodes.  A row with an index
 *   outside [0, n) or a repeated index is INVALID: it joins nothing.  label [n] int32 ends as the smallest node index of every
 *   node's component (a node no valid row touches is its own component) — a unique fixpoint, independent of scheduling.
 *   The call runs `rounds` (0 .. 64) rounds of hook + compress; rounds_done = 0 starts a run (label, parent and state are
 *   initialised, and the first round counts the invalid rows), rounds_done > 0 continues the run that has had that many
 *   rounds on the same arrays.  parent [n] int32: workspace of the run.  state [4] int32 on the device: [0] the number (from 1) of
 *   the last round that hooked anything — the labels are final as soon as state[0] is below the number of rounds run, and
 *   2 ceil(log2 n) + 2 rounds always suffice (csrc/mesh_topology.hip has the argument); [1] the invalid rows; [2], [3] zero.
 *   n = 0 or M = 0: nothing is written (every node is its own component).
 * recmv_mesh_face_stats: per face of verts [V,3] f32 / faces [F,3] int64, computed in float64: area [F] = 0.5 |(b - a) x (c - a)|,
 *   min_angle [F] = the smallest of the corner angles atan2(|u x w|, u . w) in radians, edge_ratio [F] = longest / shortest edge
 *   (inf when the shortest is 0).  An invalid face (as above, n = V): area 0, NaN, NaN.  A valid face with a corner that is not
 *   finite: NaN, NaN, NaN.  counts [2] int32 on the device: the invalid faces, the valid faces with such a corner.
 * recmv_segment_sums: values [N,C] float64 (C in 1 .. 8) whose rows are sorted by segment, offsets [S + 1] int64 (segment s is
 *   rows offsets[s] .. offsets[s + 1] - 1): sum, vmin, vmax [S,C] float64 (0, +inf, -inf for an empty segment; a NaN poisons the
 *   sum and never is a minimum or maximum).  The same bits on every run: a segment is cut into chunks of
 *   recmv_segment_sums_chunk() rows at fixed places, one wave adds a chunk (lane l the rows l, l + 64, ... in order, then a
 *   fixed shuffle tree), and a second launch adds a segment's chunk results the same way.  chunk_offsets [S + 1] int64:
 *   chunk_offsets[s] = the sum over s' < s of ceil(rows of s' / chunk).  Workspace: recmv_segment_sums_workspace_bytes(N, S, C),
 *   8-byte aligned.  Ranges read from offsets and chunk_offsets are clamped to the arrays.
 * ---------------------------------------------------------------------------------------------- */
int recmv_graph_components(int64_t n, const int64_t* links, int64_t M, int32_t K, int32_t rounds_done, int32_t rounds,
                           int32_t* label, int32_t* parent, int32_t* state, void* stream);
int recmv_mesh_face_stats(const float* verts, int64_t V, const int64_t* faces, int64_t F, double* area, double* min_angle,
                          double* edge_ratio, int32_t* counts, void* stream);
int64_t recmv_segment_sums_chunk(void);
int64_t recmv_segment_sums_workspace_bytes(int64_t N, int64_t S, int32_t C);
int recmv_segment_sums(const double* values, int64_t N, int32_t C, const int64_t* offsets, int64_t S,
                       const int64_t* chunk_offsets, double* sum, double* vmin, double* vmax, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Quadric-error edge collapse (csrc/mesh_simplify.hip; added to ABI v11, no existing signature changed).  Not in the
 * reference.  The kernels of recmv/simplify.py.  verts [V,3] f32, faces [F,3] int64; a face with an index outside [0, V) or a
 * repeated index is INVALID and contributes nothing.  Integer atomics only (counters); every float64 sum is one thread's loop
 * in table order, so results have the same bits on every run.  Argument errors (negative sizes, a weight or reach that is
 * negative or not finite, NULL pointers with work to do) are found before any HIP call; an empty input (V = 0, E = 0) is a
 * no-op that returns RECMV_OK.  Every index read from a table is checked against its array and row ranges are clamped.
 * recmv_vertex_quadrics: Q [V,11] float64 = per vertex the entries xx xy xz xw yy yz yw zz zw ww of the Garland-Heckbert
 *   quadric and a weight.  vf_offsets [V + 1] / vf_faces [n_vf] int64: vertex -> its faces, ascending; every face of the row
 *   adds area * (n, d)(n, d)^T (unit normal, plane through its first corner) and its area to the weight, in row order.
 *   border [B,3] int64 = (a, b, face): the boundary edges (used by one face) with that face; vb_offsets [V + 1] / vb_rows [n_vb]
 *   int64: vertex -> its rows of border, ascending; every one adds, after the faces, boundary_weight * |b - a|^2 * (m, d)(m, d)^T,
 *   m the unit vector of n x (b - a) (in the face's plane, perpendicular to the edge), the plane through a; nothing to the
 *   weight.  Geometry in float64 from the f32 coordinates.  A face without area or with a corner that is not finite adds
 *   nothing.  counts [1] int32 on the device: the invalid faces.
 * recmv_edge_collapse_cost: candidate edges [E,2] int64 (a, b) and code [E] uint8: 1 the vertex stays at a, 2 at b, anything else
 *   free.  With q = Q[a] + Q[b] the candidates of a free edge are, in this order, the solution of the 3x3 system (float64
 *   cofactors), a, b, the midpoint; each is rounded to f32 and its cost x^T q x evaluated in float64 at the rounded point and
 *   clamped at 0; the smallest wins, a tie goes to the earlier.  The solved point takes part only when it is finite and lies
 *   within reach * |b - a| of the midpoint.  pos [E,3] f32, cost [E] float64, weight [E] float64 = Q[a][10] + Q[b][10].  An edge
 *   with an index outside [0, V) or a == b: pos 0, the largest finite cost, weight 0; counts [1] int32 on the device counts them.
 * recmv_collapse_flip_check: ok [E] uint8 = 1 when every face of a, then of b (vf tables as above), that does not hold both
 *   ends keeps n_old . n_new > 0 with the moved end at pos [E,3] f32 (cross products in float64); 0 otherwise and for an edge
 *   as above.
 * ---------------------------------------------------------------------------------------------- */
int recmv_vertex_quadrics(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* vf_offsets,
                          const int64_t* vf_faces, int64_t n_vf, const int64_t* border, int64_t B, const int64_t* vb_offsets,
                          const int64_t* vb_rows, int64_t n_vb, double boundary_weight, double* Q, int32_t* counts,
                          void* stream);
int recmv_edge_collapse_cost(const double* Q, const float* verts, int64_t V, const int64_t* edges, int64_t E,
                             const uint8_t* code, double reach, float* pos, double* cost, double* weight, int32_t* counts,
                             void* stream);
int recmv_collapse_flip_check(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* vf_offsets,
                              const int64_t* vf_faces, int64_t n_vf, const int64_t* edges, int64_t E, const float* pos,
                              uint8_t* ok, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh smoothing (csrc/mesh_smooth.hip; added to ABI v11, no existing signature changed).  Not in the reference.  The kernels
 * of recmv/smooth.py.  verts [V,3] f32, faces [F,3] int64.  Sums in float64, one thread per output row in table order, one
 * rounding to f32 at the store, no float atomics: the same bits on every run.  Input and output are different buffers.
 * Argument errors (negative sizes, sizes of 2^31 or more, a parameter that is not finite or out of range, NULL pointers with
 * work to do) are found before any HIP call; an empty input is a no-op that returns RECMV_OK.  Every index read from a table
 * is checked against its array and row ranges are clamped.
 * Tables: nbr_offsets [V + 1] / nbr_idx [nnz] int32: vertex -> neighbour vertices, ascending; vs_offsets [V + 1] / vs_slots [n_vs]
 *   int64: vertex -> the corner slots (face * 3 + corner) that hold it, ascending; ff_offsets [F + 1] / ff_idx [nnz] int32: face
 *   -> the faces that share an edge with it, ascending, without the face itself.
 * recmv_cotan_weights: weights [nnz] float64, one per neighbour entry: w[i->j] = the sum over the faces of edge (i, j), ascending,
 *   of 1/2 max(0, cot) of the angle opposite the edge; cot at a corner = dot(e1, e2) / |cross(e1, e2)| of the edges to the next
 *   and the previous corner in the face's cyclic order, float64.  w[i->j] and w[j->i] have the same bits.  A face with an
 *   index outside [0, V), a repeated corner, a corner that is not finite or no area adds nothing; counts [1] int32 on the
 *   device counts those faces.
 * recmv_laplacian_step: out = x + lambda (sum_j w_ij x_j / sum_j w_ij - x).  weights NULL: the mean of the valid neighbours;
 *   otherwise entries that are not finite and > 0 are left out.  fixed [V] uint8 (NULL: none): copied.  No valid neighbour, or
 *   a weight sum that is not > 0: copied.  boundary_nbrs [V,2] int64 (NULL: none; -1 = none, as recmv_loop_subdivide reads
 *   it): a vertex with an entry >= 0 moves toward the midpoint of its two boundary neighbours, or is copied when it does not
 *   have two valid ones.  lambda must be finite and may be negative.
 * recmv_face_normal_filter: out [F,3] f32 = the unit vector of sum_j areas[j] exp(-|c_i - c_j|^2 / 2 sigma_c^2)
 *   exp(-|n_i - n_j|^2 / 2 sigma_s^2) n_j over the face itself, then its neighbours in row order; normals [F,3] f32, areas [F] and
 *   centroids [F,3] float64.  A face whose sum has no finite positive length keeps its normal.  sigma_c, sigma_s finite, > 0.
 * recmv_vertex_from_normals: out_i = x_i + 1/|F_i| sum_f n_f (n_f . (c_f - x_i)) over the valid faces of the vertex's slots, c_f
 *   the centroid of the face in verts; a face with a corner or normal that is not finite, or a zero normal, is left out.  A
 *   fixed vertex (NULL: none) and one without such a face are copied.
 * ---------------------------------------------------------------------------------------------- */
int recmv_cotan_weights(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* vs_offsets,
                        const int64_t* vs_slots, int64_t n_vs, const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t nnz,
                        double* weights, int32_t* counts, void* stream);
int recmv_laplacian_step(const int32_t* nbr_offsets, const int32_t* nbr_idx, int64_t V, int64_t nnz, const float* verts,
                         const double* weights, const uint8_t* fixed, const int64_t* boundary_nbrs, double lambda, float* out,
                         void* stream);
int recmv_face_normal_filter(const int32_t* ff_offsets, const int32_t* ff_idx, int64_t F, int64_t nnz, const float* normals,
                             const double* areas, const double* centroids, double sigma_c, double sigma_s, float* out,
                             void* stream);
int recmv_vertex_from_normals(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* vs_offsets,
                              const int64_t* vs_slots, int64_t n_vs, const float* normals, const uint8_t* fixed, float* out,
                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fixed-radius neighbour search over points (csrc/point_grid.hip; added to ABI v11, no existing signature changed).  Not in
 * the reference.  The kernels of recmv/repair.py (points_within, which weld joins).  verts [V,3] f32, eps >= 0 a float64.  The
 * result is every pair (i, j), i < j, of FINITE vertices with d2 <= eps * eps, d2 = (dx * dx + dy * dy) + dz * dz in float64 from
 * the f32 coordinates, no contraction: membership is exact and equals an O(V^2) loop's.  eps = 0: coincident vertices
 * (+0.0 == -0.0).  No atomics at all: the same array on every run.
 * The grid (chosen by the caller): nx x ny x nz cubic cells of edge `cell` with the corner at (ox, oy, oz), cell (x, y, z) has
 * index (z ny + y) nx + x; cell >= eps (the caller keeps cell >= eps (1 + 2^-20), which makes the 27-cell search complete under
 * float64 rounding), every axis 1 .. 2^20 cells, at most recmv_points_within_max_cells() = 2^24 in all; a coordinate outside is
 * clamped to the edge.
 * recmv_points_within_cells: cell_of [V] int32 = the cell of every vertex, -1 for a vertex with a NaN or inf coordinate.
 * The caller sorts the finite vertices by cell, by id inside a cell: pts [n,3] f32 their coordinates, ids [n] int64 their
 *   vertex ids, cell_start [cells + 1] int32 the first sorted position of every cell (cell_start[cells] = n).
 * recmv_points_within_count: counts [V] int64 = per vertex i the partners j > i (0 for a vertex that is not sorted).
 * recmv_points_within_fill: offsets [V] int64 = the exclusive scan of counts; pairs [P,2] int64 receives the rows (i, j) of
 *   vertex i from row offsets[i] on; a row outside [0, P) is not written.
 * Argument errors (negative sizes, n > V, eps or cell not finite, cell < eps, cells out of range, NULL pointers with work to do)
 * are found before any HIP call.  Values read from ids, cell_start and offsets are checked before they index anything.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_points_within_max_cells(void);
int recmv_points_within_cells(const float* verts, int64_t V, double ox, double oy, double oz, double cell, int32_t nx, int32_t ny,
                              int32_t nz, int32_t* cell_of, void* stream);
int recmv_points_within_count(const float* pts, const int64_t* ids, int64_t n, int64_t V, double eps, double ox, double oy,
                              double oz, double cell, int32_t nx, int32_t ny, int32_t nz, const int32_t* cell_start,
                              int64_t* counts, void* stream);
int recmv_points_within_fill(const float* pts, const int64_t* ids, int64_t n, int64_t V, double eps, double ox, double oy,
                             double oz, double cell, int32_t nx, int32_t ny, int32_t nz, const int32_t* cell_start,
                             const int64_t* offsets, int64_t* pairs, int64_t P, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh voxelisation (csrc/mesh_voxelize.hip; added to ABI v11, no existing signature changed).  Not in the reference.  The
 * kernels of recmv/voxelize.py: a triangle mesh (verts [V,3] f32, faces [F,3] int64, F < 2^31) turned into a distance lattice.
 * The lattice is a descriptor in HOST memory: node (i, j, k) sits at origin[a] + (float)idx[a] * step — one multiply and one
 * add in f32, not contracted — and has the index (i * ny + j) * nz + k: [NX, NY, NZ] with z contiguous, the volume layout of the
 * marching-cubes entry points.  At most 2^28 nodes (their limit); step positive and finite, the origin finite.
 * recmv_voxel_band_distance: for every node the exact nearest face among the faces within `band` of it: dist2 [N] f32 its
 *   squared distance and face [N] int64 its id, ties to the lowest id; a node with no face within the band gets +inf and -1.
 *   "Within the band": dist2 <= band * band, the product formed once in f32.  The distance is that of the closest-point entry
 *   point above (the same function on the same (a, b - a, c - a)): the same bits.  A face with an index outside [0, V) is
 *   skipped; NaN never wins.  One wave per face strides over the nodes of the face's box dilated by band and one further
 *   node; a node in the band does one 64-bit integer atomicMin on (float bits of dist2) << 32 | face id — no float atomics, and
 *   the result does not depend on the arrival order.  Workspace: recmv_voxel_band_workspace_bytes(lattice) bytes (8 per node;
 *   -1 for an unusable lattice), 8-byte aligned; it is not needed for F = 0 or V = 0.
 * recmv_voxel_sign_fill: inside [N] uint8 and sdf [N] f32 from dist2 and inside_band [N] uint8 (read at band nodes only).  One
 *   thread walks one (j, k) column along +x: a band node (dist2 <= band * band) takes inside_band, a node outside the band the
 *   value of the last band node before it in its column, outside if there is none — sound whenever band >= step, since a
 *   lattice edge the surface crosses has both ends within one step of it.  sdf = (inside ? -1 : +1) * min(sqrt(dist2), band).
 *   open_columns (one int64 in DEVICE memory) = the number of columns that end inside: 0 for a closed mesh well inside the
 *   lattice, not 0 for an open mesh or a lost parity; a diagnostic, no error.  signed_field = 0: every node is outside and
 *   inside_band is not read (it may be NULL).
 * Argument errors (NULL pointers with nodes to write, a step that is not positive and finite, a band that is negative or not
 * finite, negative dimensions, more than 2^28 nodes, a short or misaligned workspace) are found before any HIP call.  A
 * dimension of 0 is a no-op; F = 0 or V = 0 fills dist2 with +inf and face with -1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct recmv_lattice {
  float origin[3];
  float step;
  int32_t nx, ny, nz;
} recmv_lattice;
int64_t recmv_voxel_band_workspace_bytes(const recmv_lattice* lattice);
int recmv_voxel_band_distance(const float* verts, int64_t V, const int64_t* faces, int64_t F, const recmv_lattice* lattice,
                              float band, float* dist2, int64_t* face, void* workspace, int64_t workspace_bytes, void* stream);
int recmv_voxel_sign_fill(const float* dist2, const uint8_t* inside_band, const recmv_lattice* lattice, float band,
                          int signed_field, float* sdf, uint8_t* inside, int64_t* open_columns, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Hole filling (csrc/hole_fill.hip; added to ABI v11, no existing signature changed).  Not in the reference.  The kernel of
 * recmv/holes.py: the minimum-area triangulation of L closed loops in one call.  Loop l is the vertex ids
 * loop_verts[loop_offsets[l] .. loop_offsets[l+1]) (DEVICE memory, int64), n = 3 .. recmv_hole_fill_max_edges() of them, with
 * the points p_i = verts[l_i] (verts [V,3] f32; an id outside [0, V) reads as a NaN point).  Interval dynamic programming in
 * float64 on the f32 coordinates, un-contracted, every operation correctly rounded:
 *   W[i][i+1] = 0;  W[i][j] = min over i < k < j of (W[i][k] + W[k][j]) + A(i,k,j);
 *   A = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz), (cx, cy, cz) = u x v component by component (cx = u.y*v.z - u.z*v.y, ...),
 *   u = p_k - p_i, v = p_j - p_i.  A candidate wins only when it is smaller (<) than the best so far, k ascending from +inf:
 *   ties go to the lowest k, NaN never wins, an entry without a winner is +inf with k = i + 1.
 * out_weight [L] f64 = W[0][n-1] per loop (not finite: the loop has a point that is not finite).  out_faces [total - 2 L, 3]
 * int64: loop l's n - 2 faces from row loop_offsets[l] - 2 l, in pre-order of the split tree (the triangle of (i, j), then the
 * subtree of (i, k), then that of (k, j)), each written (l_j, l_k, l_i): the reverse of the loop's direction.
 * loop_offsets [L+1] is read in HOST memory (the sizes decide launches and the workspace layout) and loop_offsets_device is
 * the same array in device memory.  route: 0 auto (a loop of at most recmv_hole_fill_auto_max_edges() vertices runs in one
 * workgroup with its tables in LDS, a longer one in the workspace with one launch per diagonal), 1 every loop in LDS (a
 * loop of more than recmv_hole_fill_lds_max_edges() vertices is an argument error), 2 every loop through the workspace.  The routes give the same bits.
 * Workspace: recmv_hole_triangulate_workspace_bytes(loop_offsets, L, route) bytes, 8-byte aligned (24 B and n(n-1)/2 * 18 B
 * + 12 n B, rounded to 8, per loop that does not run in LDS; 0 when all do; -1 with a message for unusable sizes); a shorter
 * one returns RECMV_ERR_WORKSPACE.  Argument errors (L < 0, a bad route, NULL pointers, loop_offsets[0] != 0, a loop shorter
 * than 3 or longer than the cap, an output that aliases an input or the other output) are found before any HIP call.  L = 0
 * is a no-op.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_hole_fill_lds_max_edges(void);
int64_t recmv_hole_fill_auto_max_edges(void);
int64_t recmv_hole_fill_max_edges(void);
int64_t recmv_hole_triangulate_workspace_bytes(const int64_t* loop_offsets, int64_t L, int route);
int recmv_hole_triangulate(const float* verts, int64_t V, const int64_t* loop_verts, const int64_t* loop_offsets,
                           const int64_t* loop_offsets_device, int64_t L, int64_t* out_faces, double* out_weight,
                           void* workspace, int64_t workspace_bytes, int route, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Generalized winding numbers (csrc/winding.hip, csrc/solid_angle.h; added to ABI v11, no existing signature changed).  Not in
 * the reference.  The kernels of recmv/winding.py: w(q) of P points (p [P,3] f32) about a triangle mesh (verts [V,3] f32,
 * faces [F,3] int64), w [P] f64.
 * Definition.  For a face with corners A, B, C and a query q, all f32: a = A - q, b = B - q, c = C - q,
 *   Omega = 2 atan2( a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b| ),      w(q) = (sum over the faces of Omega) / 4 pi.
 *   Omega is computed in f32, un-contracted; the sum is accumulated in f64, and w = sum / 4 pi is one f64 division.  For a
 *   closed mesh w is an integer (0 outside, +-1 inside, +-2 inside two overlapping pieces), for an open one it varies smoothly;
 *   |w| > 1/2 is the inside test of recmv/winding.py (two-sided; NaN is outside).
 *   A face with an index outside [0, V) contributes 0.  A face without area contributes 0 (its numerator is 0).  A face with
 *   a corner that is not finite makes every w NaN.  A query that is not finite gets NaN.  A query exactly on a face gets
 *   2 atan2(+-0, negative) = +-2 pi for that face, a term of +-1/2.  None of these is an error.
 * Determinism.  The result of a query depends on the query and the mesh alone: not on P, on the other queries, on the launch
 *   or on scheduling.  No atomics.
 * recmv_winding_exact: every face for every query.  The faces are cut into chunks of recmv_winding_chunk_faces() faces, a
 *   constant of the library: chunk c holds the faces [c K, min(F, (c + 1) K)).  partial[c][q] = the f64 sum of chunk c's terms
 *   in ascending face order from 0., and w[q] = (((0. + partial[0][q]) + partial[1][q]) + ...) / 4 pi in ascending chunk order.
 *   The workspace holds the partials, [chunks, P] f64, and keeps them after the call:
 *   recmv_winding_exact_workspace_bytes(P, F) bytes (-1 with a message for negative sizes or more than 65535 chunks), 8-byte
 *   aligned; it is not needed for F = 0.
 * The tree route: a dense pyramid over the cube [origin, origin + side)^3 around the mesh.  Level l = 0 .. levels has 2^l
 *   cells per axis; node (l, i, j, k) is row (8^l - 1) / 7 + (i 2^l + j) 2^l + k of `nodes`, recmv_winding_tree_nodes(levels)
 *   rows of 16 floats: the area sum, the area-weighted centroid sum (3), the area-vector sum N = sum of (B - A) x (C - A) / 2
 *   (3), the number of faces (an int32's bits), the low corner of the box of the faces' corners (3), 0, the high corner (3), 0.
 *   The descriptor lies in HOST memory and its tables in device memory; levels is 1 .. 7.
 *   recmv_winding_tree_cells: cells [F] int64 = the finest cell (i n + j) n + k, n = 2^levels, of each face's centroid
 *     ((A + B) + C) / 3, an axis index being floor((x - origin) / (side / n)) clamped to [0, n - 1]; -1 for a face with an index
 *     outside [0, V) (skipped), -2 for a face with a corner that is not finite (the caller answers NaN).  Reads origin, side
 *     and levels of the descriptor only.
 *   recmv_winding_tree_build: the caller sorts the faces with a cell >= 0 by cell, stably (ascending face id within a cell):
 *     order [n_faces] int64 are their ids and cell_start [8^levels + 1] int64 the first sorted position of every finest cell.
 *     Fills tris [n_faces, 9] f32 (the sorted faces' corners) and nodes: the finest level by one thread per cell that adds
 *     its faces in sorted order, each coarser level by one thread per parent that adds its 8 children, x slowest, z fastest;
 *     f32 sums, no atomics.
 *   recmv_winding_tree_query: thread t answers query order[t] (order [P] int64, a permutation that puts neighbouring queries
 *     side by side, or NULL for the identity; an entry outside [0, P) is skipped).  Depth-first from the root in the build's
 *     child order: a node without faces is skipped; with centre = centroid sum / area sum (the box's centre when the area sum
 *     is 0), r = the largest distance from the centre to a corner of the node's box and d = centre - q, a node with
 *     |d|^2 > (beta beta) r^2 contributes N . d / |d|^3 (the first-order, dipole term); any other node is descended into, and at
 *     the finest level its faces are evaluated with the exact route's function.  f64 accumulation in visiting order, then
 *     / 4 pi.  beta is finite and at least 1; the larger, the nearer to the exact sum.
 * Argument errors (negative sizes, NULL pointers with non-zero sizes, levels outside 1 .. 7, a beta that is not finite or
 * below 1, a short or misaligned workspace, a cube side that is not positive and finite, an origin that is not finite) are
 * found before any HIP call.  P = 0 is a no-op; F = 0 writes zeros.
 * ---------------------------------------------------------------------------------------------- */
typedef struct recmv_winding_tree {
  float origin[3];
  float side;
  int32_t levels;
  int32_t reserved;
  int64_t n_faces;
  float* nodes;
  int64_t* cell_start;
  float* tris;
} recmv_winding_tree;
int64_t recmv_winding_chunk_faces(void);
int64_t recmv_winding_exact_workspace_bytes(int64_t P, int64_t F);
int recmv_winding_exact(const float* p, int64_t P, const float* verts, int64_t V, const int64_t* faces, int64_t F, double* w,
                        void* workspace, int64_t workspace_bytes, void* stream);
int64_t recmv_winding_tree_nodes(int levels);
int recmv_winding_tree_cells(const float* verts, int64_t V, const int64_t* faces, int64_t F, const recmv_winding_tree* tree,
                             int64_t* cells, void* stream);
int recmv_winding_tree_build(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* order,
                             const recmv_winding_tree* tree, void* stream);
int recmv_winding_tree_query(const float* p, int64_t P, const int64_t* order, const recmv_winding_tree* tree, float beta,
                             double* w, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Geodesic distance fields (csrc/geodesic.hip; added to ABI v11, no existing signature changed).  Not in the reference.  The
 * kernels of recmv/geodesic.py: B independent fields D [B, V] f64 over one triangle mesh (verts [V,3] f32, faces [F,3] int64).
 * Definition.  A face is usable when its three indices lie in [0, V) and are distinct and its nine coordinates are finite.
 *   For a vertex v in a usable face whose next corner (in the face's row, cyclically) is a and the one after b, with the
 *   current values Da = D(a), Db = D(b), the first-order Hopf-Lax candidate is
 *     U(v; a, b) = min over t in [0, 1] of (1 - t) Da + t Db + |v - ((1 - t) a + t b)|
 *   computed in float64 on the f32 coordinates widened to f64, un-contracted, in exactly this order (x, y, z components; a
 *   3-sum is (p + q) + r; |x| = sqrt((x0 x0 + x1 x1) + x2 x2); sqrt and / correctly rounded):
 *     w = v - a,  u = v - b,  la = |w|,  lb = |u|,  ca = Da + la,  cb = Db + lb,  U = cb < ca ? cb : ca
 *     when Da < inf and Db < inf:   e = b - a,  L2 = (e0 e0 + e1 e1) + e2 e2,  L = sqrt(L2),  delta = Db - Da
 *       when L > 0 and |delta| < L:   n = w x e = (w1 e2 - w2 e1, w2 e0 - w0 e2, w0 e1 - w1 e0),  h = |n| / L
 *         (the distance of v from the line ab, by the cross product: it does not cancel as la^2 - t0^2 L2 would)
 *         when h > 0:   t0 = ((w0 e0 + w1 e1) + w2 e2) / L2,   ts = t0 - (delta h) / (L sqrt(L2 - delta delta))
 *           when 0 < ts < 1 (false for a ts that is not finite):   r = ts - t0,
 *             ci = (Da + ts delta) + sqrt(h h + L2 (r r)),   U = ci < U ? ci : U
 *   D^0 is +inf except at the sources; D^{k+1}(v) = min(D^k(v), min over the usable faces of v of U), every U of sweep k + 1
 *   reading D^k only (Jacobi: the minimum does not depend on the order of a vertex's faces, and no update is seen early, so
 *   no bit depends on scheduling).  The answer is D^K for the least K with D^{K+1} = D^K; K is the number of sweeps.  A
 *   vertex that no usable face reaches from a source stays +inf.  In exact arithmetic K <= V.
 * The slot table: slot_offsets [V + 1] and slots int64: row v lists the corner slots 3 f + c with faces[f][c] = v (recmv.
 *   connectivity.vertex_slots_csr).  Every entry is checked against the faces; a wrong table costs wrong values only.
 * recmv_geodesic_check_sources: sources [S] int64 and values [S] f64 (or NULL: all 0) in HOST memory: RECMV_ERR_ARG with a
 *   message for a source outside [0, V) or a value that is not finite.  No HIP call at all.
 * recmv_geodesic_sweeps (any size): the workspace, recmv_geodesic_workspace_bytes(V, F, B) bytes, 8-byte aligned, is
 *   D [2][B][V] f64 | changed [2][align8(B V)] u8 | last_changed [B] int32 (padded to 8 bytes).  The caller writes D^0 into
 *   D[0]; a call runs the sweeps k0 + 1 .. k0 + n, one launch each in stream order, sweep k reading D[(k - 1) & 1] and writing
 *   D[k & 1]; the call with k0 = 0 first marks every vertex changed and clears last_changed.  A thread that lowers a value
 *   in sweep k stores k into last_changed[b] (every writer of a launch stores the same number).  After sweeps 1 .. m the
 *   field has converged when last_changed[b] < m, and then K = last_changed[b]; further sweeps change nothing.
 * recmv_geodesic_lds (V <= recmv_geodesic_lds_max_vertices() = 3640): one workgroup per field runs sweeps until one lowers
 *   nothing, D0 [B][V] -> D [B][V], sweeps [B] int32 = K, or -1 (D then holds sweep max_sweeps + 1) when sweep
 *   max_sweeps + 1 still lowered a value.  recmv_geodesic_auto_max_vertices(): up to this V recmv.geodesic's route 'auto'
 *   takes this route (measured, csrc/geodesic.hip).
 * Both routes give the bits of the definition and the same K.  Argument errors (negative sizes, sizes of 2^31 or more, NULL
 * pointers with non-zero sizes, a short or misaligned workspace, V above the lds capacity, k0, n or max_sweeps outside
 * 0 .. 2^30) return RECMV_ERR_ARG before any HIP call; V = 0 or B = 0 is a no-op.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_geodesic_lds_max_vertices(void);
int64_t recmv_geodesic_auto_max_vertices(void);
int64_t recmv_geodesic_workspace_bytes(int64_t V, int64_t F, int64_t B);
int recmv_geodesic_check_sources(const int64_t* sources, const double* values, int64_t S, int64_t V);
int recmv_geodesic_sweeps(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* slot_offsets,
                          const int64_t* slots, int64_t B, void* workspace, int64_t workspace_bytes, int64_t k0, int64_t n,
                          void* stream);
int recmv_geodesic_lds(const float* verts, int64_t V, const int64_t* faces, int64_t F, const int64_t* slot_offsets,
                       const int64_t* slots, int64_t B, const double* D0, double* D, int32_t* sweeps, int64_t max_sweeps,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh parameterisation (csrc/mesh_param.hip; added to ABI v11, no existing signature changed).  Not in the reference.  The
 * kernels of recmv/param.py: all arithmetic float64, un-contracted, + - * / sqrt only, gathers over CSR tables, no float atomics.
 * The system.  Over the neighbour CSR of recmv.connectivity.neighbours_csr (nbr_offsets [V + 1], nbr_idx [nnz] int32) with one
 *   weight per entry (the layout recmv_cotan_weights writes), an entry k of row i counts when its j = nbr_idx[k] lies in
 *   [0, V), j != i and weights[k] is finite and > 0.  d_i = the sum of the counted weights in row order.  Vertex i is active
 *   when fixed[i] == 0 and d_i > 0; a free vertex with d_i = 0 (a zero row) keeps its value and is counted in zero_rows.  For
 *   the active vertices, two columns at once (u, rhs [V,2]):
 *       (A x)_i = sum over the counted entries, in row order, of w_k (x_i - x_j)          (x_j = 0 for a j that is not active)
 *       r_i = rhs_i - sum_k w_k (u_i - u_j),   b_i = rhs_i + sum over the counted entries with fixed[j] of w_k u_j
 *   and Jacobi-preconditioned conjugate gradients from the u passed in: z = r (1 / d), p = z + beta p (beta = 0 first),
 *   q = A p, alpha = (r.z) / (p.q), u += alpha p, r -= alpha q, beta = (r.z)' / (r.z), per column; a column is active while
 *   r.r > tol^2 b.b and freezes (alpha = beta = 0) when it converges or when p.q is not > 0 or alpha / beta is not finite.  The
 *   solve ends when no column is active or after max_iter iterations.  residuals[c] = sqrt(r.r / b.b) (sqrt(r.r) when b = 0).
 * The summation order of every dot product (b.b, r.z, r.r, p.q, the zero-row count, the ARAP energy), written once: term i
 *   belongs to slot i / 256, wave (i % 256) / 64, lane i % 64; terms beyond the end and of vertices that are not active are +0.
 *   (1) a wave's 64 lanes are summed by the xor butterfly v += v[lane ^ off] for off = 32, 16, 8, 4, 2, 1; (2) a slot is
 *   ((((0 + wave 0) + wave 1) + wave 2) + wave 3); (3) with T = 256 accumulators, accumulator t adds the slots t, t + 256, ...
 *   in that order from 0; (4) the 256 accumulators are summed like one slot: butterflies over 64, then the four from 0.
 *   (mesh_device.h's block_partials and reduce_slots.)  Both routes follow it, so they give the same bits and iteration count.
 * recmv_param_solve (any V): workspace of recmv_param_solve_workspace_bytes(V) bytes, 256-byte aligned.  Two launches per
 *   iteration, queued `batch` (<= 0: 32) iterations at a time with one small launch and one read-back of the state per batch;
 *   the batch size changes no bit.  iterations, residuals [2] and zero_rows are HOST pointers.  The call synchronises.
 * recmv_param_solve_lds (V <= recmv_param_lds_max_vertices() = (163840 - 4096) / 72 = 2218): the whole solve in one launch by
 *   one workgroup, u, r, p, q and 1 / d in LDS.  `report`: at least 128 bytes of DEVICE memory, 8-byte aligned.
 *   recmv_param_auto_max_vertices(): up to this V recmv.param's route 'auto' takes this route.
 * recmv_param_face_frames: per face the isometric flattening, frames [F,4] = (x1, x2, y2, area): corner 0 at (0, 0), corner 1
 *   at (x1, 0) with x1 = |e1|, corner 2 at (x2, y2) = (e1.e2 / x1, |e1 x e2| / x1), area = |e1 x e2| / 2 (e1 = p1 - p0,
 *   e2 = p2 - p0); and cots [F,3]: 1/2 max(0, cot) at each corner, recmv_cotan_weights' expression.  A face is usable when its
 *   indices are distinct and in [0, V), its corners finite and |e1 x e2| finite and > 0; an unusable face gets zeros.
 * recmv_param_arap_rhs: with X the flat corners, half-edge k of a face runs from corner a = k + 1 to b = k + 2 (mod 3) with the
 *   weight c_k = cots[k].  S = sum_k c_k (u_a - u_b)(X_a - X_b)^T, (a, b) = (S00 + S11, S10 - S01) / its length ((1, 0) when the
 *   length is 0 or not finite) -> rot [F,2], the rotation R = [[a, -b], [b, a]]; the face's energy sum_k c_k |(u_a - u_b) -
 *   R (X_a - X_b)|^2 -> partials [(F + 255) / 256] in the order above and their sum -> energy [1].  Then per vertex over the
 *   slot table (slot_offsets [V + 1], slots: recmv.connectivity.vertex_slots_csr, every entry checked against the faces), for
 *   corner k of a usable face: rhs_i += c_{k+2} R (X_k - X_{k+1}), then rhs_i += c_{k+1} R (X_k - X_{k+2}).  Unusable faces
 *   (area 0 in frames, or indices that are not valid) add nothing.
 * recmv_param_distortion: out [F,3] = (s1, s2, det) of the Jacobian J of the map flat triangle -> uv:
 *   J00 = a0 / x1, J10 = a1 / x1, J01 = (b0 - J00 x2) / y2, J11 = (b1 - J10 x2) / y2 with a = uv1 - uv0, b = uv2 - uv0;
 *   E = (J00 + J11) / 2, F = (J00 - J11) / 2, G = (J10 + J01) / 2, H = (J10 - J01) / 2, Q = sqrt(E E + H H), R = sqrt(F F + G G),
 *   s1 = Q + R, s2 = |Q - R|, det = J00 J11 - J01 J10.  An unusable face gives NaN, NaN, 0.
 * Argument errors (negative sizes, sizes of 2^31 or more, NULL pointers with non-zero sizes, a short or misaligned workspace, V
 * above the lds capacity, tol < 0 or NaN, max_iter < 0) return RECMV_ERR_ARG before any HIP call; empty inputs are no-ops.
 * ---------------------------------------------------------------------------------------------- */
int64_t recmv_param_lds_max_vertices(void);
int64_t recmv_param_auto_max_vertices(void);
int64_t recmv_param_solve_workspace_bytes(int64_t V);
int recmv_param_solve(const int32_t* nbr_offsets, const int32_t* nbr_idx, const double* weights, int64_t V, int64_t nnz,
                      const uint8_t* fixed, const double* rhs, double* u, double tol, int32_t max_iter, int32_t batch,
                      int32_t* iterations, double* residuals, int32_t* zero_rows, void* workspace, int64_t workspace_bytes,
                      void* stream);
int recmv_param_solve_lds(const int32_t* nbr_offsets, const int32_t* nbr_idx, const double* weights, int64_t V, int64_t nnz,
                          const uint8_t* fixed, const double* rhs, double* u, double tol, int32_t max_iter,
                          int32_t* iterations, double* residuals, int32_t* zero_rows, void* report, void* stream);
int recmv_param_face_frames(const float* verts, int64_t V, const int64_t* faces, int64_t F, double* frames, double* cots,
                            void* stream);
int recmv_param_arap_rhs(const int64_t* faces, int64_t F, const double* frames, const double* cots, const double* uv, int64_t V,
                         const int64_t* slot_offsets, const int64_t* slots, double* rot, double* rhs, double* partials,
                         double* energy, void* stream);
int recmv_param_distortion(const int64_t* faces, int64_t F, const double* frames, const double* uv, int64_t V, double* out,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * Texture baking (csrc/texture_bake.hip; added to ABI v11, no existing signature changed).  Not in the reference.  The kernels of
 * recmv/bake.py.  Coverage and barycentrics are float64, un-contracted; attributes are mixed in float32 in a fixed order; the only
 * atomics are integer.  Images are row-major [H,W]; uv [V,2] float64, faces [F,3] int64.
 * The coverage rule.  Texel (row y, column x) has its centre at px = (x + 0.5) / W, py = ((H - y) - 0.5) / H (row 0 is v = 1).
 *   For a directed edge a -> b with lo = min(a, b), hi = max(a, b) by vertex index:
 *       E = (u_hi - u_lo) (py - v_lo) - (v_hi - v_lo) (px - u_lo), negated if a > b.
 *   A = the edge function of i0 -> i1 at vertex i2.  A face whose indices are not distinct and in [0, V), or whose A is 0 or
 *   not finite, covers nothing; A < 0 (flipped in the UV plane) negates its three E.  A face covers a centre iff E12 >= 0,
 *   E20 >= 0 and E01 >= 0 (edges i1 -> i2, i2 -> i0, i0 -> i1) AND the texel lies in the face's box: columns
 *   max(0, floor(umin W - 0.5)) .. min(W - 1, ceil(umax W - 0.5)), rows max(0, floor(H - 0.5 - vmax H)) ..
 *   min(H - 1, ceil(H - 0.5 - vmin H)), evaluated in float64 as written, left to right.  The owner of a texel is the lowest
 *   covering face id, count the number of covering faces, S = (E12 + E20) + E01 and bary = (E12 / S, E20 / S, E01 / S) cast to
 *   float32; a texel without an owner has face -1 and bary 0.
 * recmv_bake_raster: face [H,W] int32 (also the owner image: preset to INT32_MAX, atomicMin, resolved in place), bary [H,W,3]
 *   float32, count [H,W] int32 (atomicAdd).  lanes = 8 or 64 threads per face walk its box; the launch shape changes no bit.
 * recmv_bake_gutter: src [H,W] int32.  A covered texel (face >= 0) maps to its own linear index y W + x.  In pass k = 1 ..
 *   passes a still-empty texel takes the src of the first neighbour filled before pass k, tried in the order W (x - 1), E
 *   (x + 1), N (y - 1), S (y + 1), NW, NE, SW, SE; texels still empty afterwards hold -1.  scratch: a second [H,W] int32 image
 *   (may be NULL when passes = 0).
 * recmv_bake_pad: out [T,C] = image[src[i]] (zeros where src is not in [0, T)); out must not alias image.
 * recmv_bake_interpolate: out [T,C] (1 <= C <= 16), out[c] = (b0 a0[c] + b1 a1[c]) + b2 a2[c] in float32 with a_k the attribute
 *   row of corner k of faces[face[i]]; zeros where face[i] is not a valid face.  normalise (C >= 3): the first three channels
 *   (x, y, z) widened to float64 and divided by sqrt((x x + y y) + z z), cast back; a vector without a finite positive length
 *   stays as it is.
 * recmv_bake_transfer: for hit i = (src_face[i], src_point[i]) on the source mesh, with p0, p1, p2 the face's float32 corners
 *   widened to float64, e1 = p1 - p0, e2 = p2 - p0, d = p - p0, dots as (x0 y0 + x1 y1) + x2 y2:
 *       det = (e1.e1)(e2.e2) - (e1.e2)(e1.e2);  b1 = ((e2.e2)(d.e1) - (e1.e2)(d.e2)) / det;  b2 = ((e1.e1)(d.e2) - (e1.e2)(d.e1)) / det;
 *       b0 = (1 - b1) - b2;   det not finite or not > 0 (a degenerate source face): (1, 0, 0).
 *   bary [T,3] = the three cast to float32, out [T,C] = the mix above of the source attribute; a src_face that is no valid
 *   face gives zeros in both.
 * recmv_bake_vertex_tangents: out [V,4] float32.  Per vertex over the (face, corner) codes of recmv.shading.
 *   vertex_face_adjacency (adj_offsets [V + 1], adj_codes [3F] int32) in their order, float64: a face with A (above) 0 or not
 *   finite, or with a 3-D area 1/2 |e1 x e2| that is not finite and > 0, adds nothing; otherwise with w = area / A,
 *   T += w (e1 dv2 - e2 dv1), B += w (e2 du1 - e1 du2) (du_k, dv_k = uv_k - uv_0).  t = T - n (n.T) with n the vertex normal,
 *   normalised; handedness = -1 if cross(n, t).B < 0 else +1.  No usable face or no finite positive length: (0, 0, 0, 1).
 * recmv_bake_encode_normal: out [T,3] = 0.5 + 0.5 (N.t', w N.(n x t'), N.n) with N = normal [T,3], n = frame_n [T,3], (t, w') =
 *   frame_t [T,4], w = -1 if w' < 0 else +1, t' = (t - n (n.t)) / its length (t itself when that length is not finite and > 0):
 *   the interpolated tangent made orthogonal to the interpolated normal again; float64 from the float32 inputs, cast back;
 *   zeros where face[i] < 0.
 * Argument errors (negative sizes, sizes of 2^31 or more, lanes other than 8 and 64, C outside 1 .. 16, NULL pointers with
 * non-zero sizes) return RECMV_ERR_ARG before any HIP call; empty inputs are no-ops.
 * ---------------------------------------------------------------------------------------------- */
int recmv_bake_raster(const double* uv, int64_t V, const int64_t* faces, int64_t F, int64_t H, int64_t W, int32_t lanes,
                      int32_t* face, float* bary, int32_t* count, void* stream);
int recmv_bake_gutter(const int32_t* face, int64_t H, int64_t W, int32_t passes, int32_t* src, int32_t* scratch, void* stream);
int recmv_bake_pad(const float* image, const int32_t* src, int64_t T, int32_t C, float* out, void* stream);
int recmv_bake_interpolate(const int32_t* face, const float* bary, int64_t T, const int64_t* faces, int64_t F, const float* attr,
                           int64_t V, int32_t C, int32_t normalise, float* out, void* stream);
int recmv_bake_transfer(const int64_t* src_face, const float* src_point, int64_t T, const float* src_verts, int64_t V,
                        const int64_t* src_faces, int64_t F, const float* attr, int32_t C, int32_t normalise, float* bary,
                        float* out, void* stream);
int recmv_bake_vertex_tangents(const float* verts, const double* uv, const float* normals, int64_t V, const int64_t* faces,
                               int64_t F, const int32_t* adj_offsets, const int32_t* adj_codes, float* out, void* stream);
int recmv_bake_encode_normal(const int32_t* face, const float* normal, const float* frame_n, const float* frame_t, int64_t T,
                             float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RECMV_HIP_H_ */
