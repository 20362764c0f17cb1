/*
 * include/usip_hip.h -- C ABI of libusip_hip.so, the MI355X (gfx950) implementation of the
 * USIP detector hot path.  This is the drop-in boundary: plain pointers and sizes, no torch
 * types.  The reference reaches the same operators through two pybind11/torch extensions and
 * through ATen calls in its Python modules; each entry point below cites what it replaces
 * (paths relative to the reference checkout).
 *
 * Conventions (all entry points)
 *   - every pointer is a DEVICE pointer on the current HIP device unless the name ends in
 *     `_cpu`; buffers are caller-owned, contiguous, row-major, and never aliased;
 *   - nothing is allocated, nothing synchronises: kernels are enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the legacy default stream) and the call returns;
 *   - return value: 0 on success, USIP_EINVAL for a bad argument, otherwise the hipError_t
 *     of the failed launch (positive);
 *   - outputs are fully written (callers need not pre-zero them) unless stated;
 *   - int32 indices, fp32 values; index outputs are bit-exact with the reference, float outputs
 *     agree to fp32 rounding (<= 1e-5 relative).
 */
#ifndef USIP_HIP_H
#define USIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define USIP_OK      0
#define USIP_EINVAL (-1)
/* Counts incompatible changes of this file; usip_version() reports it as "abi=<n>" and usip_amd/_lib.py, which reads the
 * signatures, the structs and this number from this file, refuses a library that reports another (a bare decimal literal). */
#define USIP_ABI 6

/* Library identification: "usip_hip <version> gfx950 abi=<USIP_ABI> flags=<...>". */
const char* usip_version(void);

/* Launch-geometry knobs for measurement sweeps (tools/): they change HOW a result is computed (rows per
 * workgroup, prefetch depth, tile order), never the result.  0 restores the library's heuristic.  No reference
 * counterpart.  Returns USIP_EINVAL for an unknown name. */
/* "x2_direct" (USIP_TUNE_X2_DIRECT) chooses among the f32x2 GEMMs of the 256..640-wide layers.  Its whole value set is 0, 1, 8
 * and 12; each value other than 0 is kept because tests take their reference from it (every other value acts as 12):
 *    0 = the product: csrc/gemm_x2f.hip (one wave per SIMD, 256 x 256 tiles) wherever a launch fits it, csrc/gemm_x2d.hip for
 *        what it refuses -- K tails, partial tiles, stage counts that are no multiple of 4: a selection by the input;
 *    1 = the LDS-staged gemm_x3p_kernel<.., 4, 2, 2> of round 3 instead of either: also the only kernel for clouds of
 *        K * P * 4 >= 2^31 bytes, and the reference of test_direct_gemm_forward_is_fp32_accurate;
 *    8 = csrc/gemm_x2d.hip with the LDS-transposing epilogue for data gradients too: the reference of
 *        test_data_gradient_stores_straight_from_the_registers_at_chip_filling_size;
 *   12 = csrc/gemm_x2d.hip only, never csrc/gemm_x2f.hip: the reference of the gemm_x2f bit-identity test and of the
 *        profiling-key test.
 * The forms that lost their measurement are gone together with the values that selected them (one stage of loads in flight, one
 * tile per workgroup, the all-DMA forward kernel, the prologue subsets of gemm_x2f, the time-split aid: profiles/HISTORY.md).
 * The REDK form of gemm_x2d.hip (usip_mlp_gemm_x2h_red_f32, off by default, measured slower) stays as the only working form
 * of an idea the project still wants, with the only test of its arithmetic; it is chosen by its own entry point, not by a knob.
 * "r5_forms" (USIP_TUNE_R5_FORMS), bit flags that bring back round 4's form of a kernel for same-box A/B runs: 1 = the f32x2
 * weight gradient with half-line loads (wgrad_x3_kernel<.., 2> instead of wgrad_x2l_kernel); and that switch ON forms round 5
 * measured and did not keep: 2 / 4 = two / four loop iterations' loads in flight in the BatchNorm-backward reduction (default
 * one), 8 = several batches of rows per workgroup with prefetch in group_max4 (default one); 32 = the 128-row-tile split GEMM with
 * round 4's two-slot weight ring (DMA one stage ahead, issued at the top of the stage) instead of the three-slot one;
 * 64 = narrow_fwd with 1024 / 768 workgroups; 128 = usip_knn_layer_backward_f32 with one row and 256 threads per workgroup (default: two rows, 512 threads). */
enum { USIP_TUNE_INDEX_MAX_CH = 0, USIP_TUNE_INDEX_MAX_UNROLL, USIP_TUNE_X3_WGRAD_TILE, USIP_TUNE_X3_GEMM_TILE,
       USIP_TUNE_GEMM_SPLIT3, USIP_TUNE_INDEX_MAX_THREADS, USIP_TUNE_X2_DIRECT, USIP_TUNE_R5_FORMS, USIP_TUNE_COUNT };
int usip_set_tuning(const char* name, int value);
int usip_tuning_value(int knob);

/* Which kernels did a call launch?  usip_launch_log(1) arms (and empties) the calling thread's log, usip_launch_log(0)
 * switches it off; both return the number of launches it held.  While armed, every kernel launch the library makes from
 * that thread is recorded (the first 8).  usip_launch_log_entry(i, &wg): the demangled name of launch i's kernel, as a
 * rocprofv3 kernel trace prints it ("void (anonymous namespace)::gemm_x2f_kernel<1, 1, false>(...)"), valid until the
 * thread's next call, and its number of workgroups; NULL when there is no entry i.  No reference counterpart. */
int usip_launch_log(int on);
const char* usip_launch_log_entry(int i, unsigned* workgroups);

/* ------------------------------------------------------------------ a-1  index_max
 * Replaces index_max.forward_cuda / forward_cuda_shared_mem
 * (models/index_max_ext/index_max.cpp:132-148 -> index_max_cuda.cu:9-25, :29-61, :65-98).
 *   max_idx[b,c,k] = lowest n with index[b,n]==k attaining max data[b,c,n], provided that
 *   maximum is strictly greater than -1000; otherwise (empty node, sub-floor values, NaN) 0.
 * data f32 [B,C,N], index i32 [B,N] with values in [0,K), max_idx i32 [B,C,K] (fully written).
 * Lifts the reference's limits (B <= 1024 threads, B*K*4 <= 48 KB shared memory). */
int usip_index_max_f32(const float* data, const int32_t* index, int32_t* max_idx,
                       int B, int C, int N, int K, void* stream);
/* The launch geometry usip_index_max_f32 / usip_index_max_values_f32 choose for a shape (knobs applied): channel rows per
 * workgroup, prefetch depth, threads per workgroup.  Host arithmetic only; lets a benchmark name the launch it times. */
int usip_index_max_geometry(int B, int C, int N, int K, int* channel_rows, int* prefetch_depth, int* threads);

/* Host twins: index_max.forward_cpu (index_max.cpp:73-112) and forward_multi_thread_cpu
 * (index_max.cpp:33-70; channels split over num_threads std::threads).  HOST pointers. */
int usip_index_max_f32_cpu(const float* data, const int32_t* index, int32_t* max_idx,
                           int B, int C, int N, int K, int num_threads);

/* ------------------------------------------------------------------ a-2  ball_query
 * Replaces ball_query.forward_cuda_shared_mem
 * (models/ball_query_ext/ball_query.cpp:33-39 -> ball_query_cuda.cu:10-49, :53-70).
 *   per (b,m): the first K indices n (ascending) with dist[b,m,n] <= radius; if 0 < u < K hits,
 *   out[u+i] = out[i % u]; if u == 0 the row is all zeros.
 * dist f32 [B,M,N], out_idx i32 [B,M,K] (fully written). radius is a C float as in the kernel. */
int usip_ball_query_f32(const float* dist, int32_t* out_idx, float radius, int K,
                        int B, int M, int N, void* stream);

/* Host twin (HOST pointers, no stream): the same rows for BASELINE configs[0], the reference's CPU plumbing case.  The
 * reference itself has no CPU ball_query (models/ball_query_ext/ball_query.cpp:23-31 is a stub). */
int usip_ball_query_f32_cpu(const float* dist, int32_t* out_idx, float radius, int K, int B, int M, int N);

/* ------------------------------------------------------------------ pairwise distances
 * Replaces the materialised torch.norm(a.unsqueeze(3) - b.unsqueeze(2), dim=1) in front of
 * ball_query (models/networks.py:694-696, :355-357):
 *   dist[b,m,n] = sqrt(fma(dz,dz, fma(dy,dy, dx*dx))), d* = a[b,*,m] - x[b,*,n]
 * (the arithmetic order of the pinned oracle platform, bit-exact with it).
 * a f32 [B,3,M], x f32 [B,3,N] -> dist f32 [B,M,N]. */
int usip_pairwise_dist_f32_cpu(const float* a, const float* x, float* dist, int B, int M, int N);   /* host twin */
int usip_pairwise_dist_f32(const float* a, const float* x, float* dist,
                           int B, int M, int N, void* stream);

/* f-2  Fused coords-in ball query: same result as usip_pairwise_dist_f32 followed by
 * usip_ball_query_f32, without ever writing the B x M x N matrix. */
int usip_ball_query_coords_f32(const float* node, const float* x, int32_t* out_idx, float radius,
                               int K, int B, int M, int N, void* stream);

/* ------------------------------------------------------------------ a-3 / a-4  SOM front end
 * Replaces util/som.py:31-54 (query_topk with k = 1) and models/networks.py:85-108.
 *   min_idx[b,n] = argmin_m (dx*dx + dy*dy) + dz*dz   (first minimum; squared distance summed
 *                  in channel order without FMA, as ATen's pow-then-sum does)
 * x f32 [B,3,N], node f32 [B,3,M] -> min_idx i32 [B,N].  The reference's dense one-hot `mask`
 * [B,N,M] is never built; `mask_row_max` is (count > 0). */
int usip_som_assign_f32(const float* x, const float* node, int32_t* min_idx,
                        int B, int N, int M, void* stream);

/* cluster_mean[b,:,m] = sum_{n: min_idx[b,n]==m} x[b,:,n] / (count[b,m] + 1e-5)  (networks.py:95-96),
 * count i32 [B,M], and (if x_decentered != NULL) x_decentered[b,:,n] = x - cluster_mean[.., min_idx]
 * (networks.py:103-107).  Deterministic (fixed-order) summation. */
int usip_som_cluster_f32(const float* x, const int32_t* min_idx, float* cluster_mean,
                         int32_t* count, float* x_decentered, int B, int N, int M, void* stream);
/* The same outputs from min_idx sorted by node (usip_csr_by_index_i32 below with P = N points, N = M nodes):
 * O(N) per cloud instead of every node scanning all assignments. */
int usip_som_cluster_csr_f32(const float* x, const int32_t* min_idx, const int32_t* start, const int32_t* perm,
                             float* cluster_mean, int32_t* count, float* x_decentered, int B, int N, int M,
                             void* stream);

/* index_max together with what the reference does with its result (models/networks.py:117-118, :130-131:
 * torch.gather at the arg-max, times mask_row_max): max_val[b,c,k] = count[b,k] > 0 ? data[b,c,max_idx[b,c,k]] : 0
 * (count NULL: every node counts as populated).  data is the channel slice [0, C) of a [B][Ctot][N] tensor.
 * max_idx as usip_index_max_f32, bit for bit (same kernel). */
int usip_index_max_values_f32(const float* data, const int32_t* index, const int32_t* count, int32_t* max_idx,
                              float* max_val, int B, int C, int Ctot, int N, int K, void* stream);
/* Backward of that gather + mask, ADDED into an existing dense gradient: ddata[b][coff+c][max_idx[b,c,k]] += g[b,c,k]
 * for populated nodes.  ddata [B][Ctot][N]. */
int usip_index_max_values_backward_add_f32(const float* g, const int32_t* max_idx, const int32_t* count, float* ddata,
                                           int B, int C, int Ctot, int coff, int N, int K, void* stream);
/* The same gradient as one dense, contiguous tensor: dz[b][c][n] = (src ? src[b][soff+c][n] : 0) + that scatter term,
 * every element written once (index = the assignment index_max was given; src [B][Csrc][N] or NULL; K <= 8192). */
int usip_index_max_values_backward_f32(const float* g, const int32_t* max_idx, const int32_t* count,
                                       const int32_t* index, const float* src, int Csrc, int soff, float* dz,
                                       int B, int C, int N, int K, void* stream);

/* ------------------------------------------------------------------ a-4 / a-12  index tensors sorted by destination
 * idx i32 [B][P] with values in [0, N) -> start i32 [B][N+1], perm i32 [B][P]: perm[b][start[b][n] .. start[b][n+1])
 * are the positions p with idx[b][p] == n (values outside [0, N) are left out; start[b][N] = number placed).
 * One counting sort per cloud; N <= 1820.  Every scatter-add of the path (torch.gather's backward in
 * models/layers.py:422-426 and networks.py:119-125, the cluster sums of networks.py:87-107) becomes a gather over
 * these segments: no float atomics, a fixed summation order. */
int usip_csr_by_index_i32(const int32_t* idx, int32_t* start, int32_t* perm, int B, int P, int N, void* stream);
/* dx[b][c][n] = sum_{j in segment n} src[b][coff+c][perm[b][j]]; src [B][Ctot][P], dx [B][C][N] (fully written).
 * P <= 16384 (a source row is staged in LDS): usip_segment_sum_supported. */
int usip_segment_sum_supported(int N, int P);
int usip_segment_sum_f32(const float* src, const int32_t* start, const int32_t* perm, float* dx,
                         int B, int C, int N, int P, int Ctot, int coff, void* stream);

/* ------------------------------------------------------------------ a-9 / a-10  chamfer core
 * min_d[b,i] = min_j |a[b,:,i] - b[b,:,j]|_2 and arg[b,i] = FIRST j attaining it, exactly what
 * torch.min(torch.norm(a.unsqueeze(3) - b.unsqueeze(2), dim=1), dim=2) returns
 * (models/losses.py:62-66, :81, :86, :135-143) without materialising the B x Ma x Nb matrix.
 * a f32 [B,3,Ma], b f32 [B,3,Nb] -> min_d f32 [B,Ma], arg i32 [B,Ma].  With few queries and many candidates
 * the candidate set is split over workgroups; ws_d / ws_j hold the per-chunk results
 * (usip_nearest_workspace elements each; NULL = single-chunk kernel). */
long long usip_nearest_workspace(int B, int Ma, int Nb);   /* elements of ws_d AND of ws_j (0: none needed) */
int usip_nearest_f32(const float* a, const float* b, float* min_d, int32_t* arg,
                     float* ws_d, int32_t* ws_j, int B, int Ma, int Nb, void* stream);
/* Its backward (what autograd derives through torch.norm + torch.min + gather in the reference):
 * ga[b][:][i] = gd[b][i] * (a_i - b_J) / d, zero where d == 0; gb (may be NULL; every element is
 * written) receives the negative summed over the queries that share a partner -- a deterministic segmented
 * sum, not float atomics. */
int usip_nearest_backward_f32(const float* a, const float* b, const float* d, const int32_t* arg,
                              const float* gd, float* ga, float* gb, int B, int C, int Ma, int Nb, void* stream);

/* ------------------------------------------------------------------ cell grid: the same two searches without the pairs
 * (csrc/cell_grid.hip).  usip_cell_grid_build_f32 sorts every cloud of x f32 [B,3,N] into a uniform 3-D grid over the
 * bounding box of its points, cell edge >= `edge` (grown until the grid has at most usip_cell_grid_cap() cells):
 *   hdr        i32 [B][USIP_CELL_HDR_WORDS]       the words below (floats as their bits)
 *   cell_start i32 [B][usip_cell_grid_cap() + 1]  first sorted position of every cell, x fastest; [cells] = N
 *   pts        f32 [B][N][4], 16-B aligned        the points in cell order: x, y, z, and the point's index as its bits
 * USABLE is 0 -- and the rest of that cloud's grid unwritten -- for a cloud with a non-finite coordinate or an extent that
 * is not finite, N = 0 or N > 2^20, an edge that is not finite or below 2^-50, or (max_block > 0) a dense cloud: one whose
 * 27-cell blocks hold more than max_block points on average, N * 27 / cells; such a cloud is not sorted at all, its rows
 * scan.  For a ball query with K samples max_block = sqrt(N * K) states the row rule below for the whole cloud.  The searches read the header on the
 * device: nothing here allocates, synchronises or reads device data on the host. */
#define USIP_CELL_HDR_WORDS 12
enum { USIP_CELL_OX = 0, USIP_CELL_OY = 1, USIP_CELL_OZ = 2, USIP_CELL_EDGE = 3, USIP_CELL_INV = 4, USIP_CELL_NX = 5,
       USIP_CELL_NY = 6, USIP_CELL_NZ = 7, USIP_CELL_USABLE = 8 };
#define USIP_CELL_CAP 15360
enum { USIP_ROUTE_SCAN = 0, USIP_ROUTE_GRID = 1 };
int usip_cell_grid_cap(void);
float usip_cell_grid_edge_factor(void);          /* 1.03125: ask for edge = radius * this for a ball query of that radius */
int usip_cell_grid_hdr_word(const char* name);   /* "ox" "oy" "oz" "edge" "inv" "nx" "ny" "nz" "usable" -> word; "words" -> count */
int usip_cell_grid_build_f32(const float* x, float edge, int max_block, int32_t* hdr, int32_t* cell_start, float* pts,
                             int B, int N, void* stream);
/* usip_ball_query_coords_f32's rows, bit for bit, from the points of the 27 cells around every node.  The grid must be the
 * one built from this x with edge = radius * usip_cell_grid_edge_factor() or more (the kernel insists on radius * 1.015625;
 * csrc/cell_grid.h says why); a row whose cloud is not
 * USABLE or has a narrower edge, or whose 27 cells hold more than 512 points or more than sqrt(N * K) (the index-order
 * scan with its exit after K hits is then the shorter one), is scanned in index order by the same launch.
 * route (may be NULL): u8 [B,M], USIP_ROUTE_GRID or USIP_ROUTE_SCAN per row. */
int usip_ball_query_grid_f32(const float* node, const float* x, const int32_t* hdr, const int32_t* cell_start,
                             const float* pts, int32_t* out_idx, uint8_t* route, float radius, int K, int B, int M, int N,
                             void* stream);
/* usip_nearest_f32's (min_d, arg), bit for bit, for a f32 [B,3,Ma] against the gridded x f32 [B,3,N] (any edge): blocks of
 * 3^3, 5^3, 7^3 cells around the query's cell until no point outside the block can be the answer; a query
 * that is not settled by then or whose block holds more than 1024 points, and every query of a cloud that is not USABLE,
 * is scanned in index order by the same launch.
 * route (may be NULL): u8 [B,Ma]. */
int usip_nearest_grid_f32(const float* a, const float* x, const int32_t* hdr, const int32_t* cell_start,
                          const float* pts, float* min_d, int32_t* arg, uint8_t* route, int B, int Ma, int N, void* stream);

/* a-8 / a-11: the element-wise tail of the step, one launch each way per line of the reference (csrc/head.hip).
 * keypoints[b][:][m] = ks[b][0:3][m] + centre[b][:][m];  sigmas[b][m] = softplus(ks[b][3][m]) + sigma_lower_bound
 * (models/networks.py:150-154; torch.nn.Softplus defaults).  ks [B][4][M], centre [B][3][M]. */
int usip_detector_head_f32(const float* ks, const float* centre, float sigma_lower_bound, float* keypoints,
                           float* sigmas, int B, int M, void* stream);
/* g_ks [B][4][M] from g_keypoints [B][3][M] and g_sigmas [B][M] (either may be NULL = zero). */
int usip_detector_head_backward_f32(const float* g_keypoints, const float* g_sigmas, const float* ks, float* g_ks,
                                    int B, int M, void* stream);
/* out[b] = (R[b] * scale[b]) . x[b] + shift[b]  (models/keypoint_detector.py:182-184: R.kp*s + t), x/out [B][3][M],
 * R [B][3][3], scale [B], shift [B][3].  transpose != 0: out[b] = (R[b] * scale[b])^T . x[b] (its backward; shift unused). */
int usip_rigid_transform_f32(const float* x, const float* R, const float* scale, const float* shift, float* out,
                             int transpose, int B, int M, void* stream);
/* out3 = (chamfer[0] + alpha * (mean(d[0:half]) + mean(d[half:2*half])), alpha * mean(first), alpha * mean(second)):
 * the sum of the step's losses (keypoint_detector.py:196-204); means in double. */
int usip_detector_loss_combine_f32(const float* d, const float* chamfer, float alpha, float* out3, long long half,
                                   void* stream);
/* out[0:n] = g[0] * factor (the gradient of a mean). */
int usip_fill_scaled_f32(const float* g, float factor, float* out, long long n, void* stream);

/* The loss segment of the detector step, keypoints / sigmas to their gradients, in three launches (csrc/loss_tail.hip)
 * instead of the chain rigid_transform, 2 x nearest, chamfer_prob, loss_combine and their backwards with what autograd
 * launches around them.  Same arithmetic, operation for operation: every result equals the chain's bit for bit.
 * keypoints f32 [2B][3][M] and sigmas f32 [2B][M] hold the src clouds in rows [0,B) and the dst clouds in [B,2B);
 * R [B][3][3], scale [B], shift [B][3].  1 <= M <= 1024 (a pair is staged in LDS) and 1 <= B <= 65535; anything else,
 * or a NULL pointer, is USIP_EINVAL with nothing launched (callers then run the chain).
 * scan: kp_t [B][3][M] = (R scale) . keypoints_src + shift; (a, J) [B][M] = usip_nearest_f32(kp_t, keypoints_dst),
 * (c, I) [B][M] = usip_nearest_f32(keypoints_dst, kp_t).  One launch. */
int usip_loss_tail_scan_f32(const float* keypoints, const float* R, const float* scale, const float* shift, float* kp_t,
                            float* a, int32_t* J, float* c, int32_t* I, int B, int M, void* stream);
/* sums: out6 = (loss, loss_chamfer, chamfer_pure, chamfer_weighted, alpha * mean(d[0:B]), alpha * mean(d[B:2B])) with
 * the middle three as usip_chamfer_prob_f32 and the others as usip_detector_loss_combine_f32; d f32 [2B][M] are the
 * keypoint-to-cloud distances.  One launch of one workgroup. */
int usip_loss_tail_sums_f32(const float* a, const int32_t* J, const float* c, const int32_t* I, const float* sigmas,
                            const float* d, float alpha, float* out6, int B, int M, void* stream);
/* backward: g_keypoints [2B][3][M] and g_sigmas [2B][M] (every element written) for the upstream gradient gloss[0] of
 * the loss.  (d, arg) [2B][M] are the keypoint-to-cloud minima against pc f32 [2B][3][N]; factor = alpha / (B * M) as
 * a float, the factor usip_fill_scaled_f32 is given for the same gradient.  One launch, no atomics. */
int usip_loss_tail_backward_f32(const float* gloss, const float* keypoints, const float* sigmas, const float* kp_t,
                                const float* a, const int32_t* J, const float* c, const int32_t* I, const float* d,
                                const int32_t* arg, const float* pc, const float* R, const float* scale, float factor,
                                float* g_keypoints, float* g_sigmas, int B, int M, int N, void* stream);

/* ------------------------------------------------------------------ a-11  optimizer.step()
 * One Adam step (models/keypoint_detector.py:42-45, :207: torch.optim.Adam(lr, betas = (0.9, 0.999)), eps 1e-8, no
 * weight decay) on flat fp32 buffers of n elements, 16-B aligned: step_count[0] += 1 (device float, so the update can
 * live in a captured HIP graph), then m = lerp(m, g, 1 - b1), v = b2 v + (1 - b2) g^2,
 * p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps) -- the arithmetic of torch's single-tensor update. */
int usip_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* step_count,
                       float lr, float beta1, float beta2, float eps, long long n, void* stream);
/* The same with (lr, beta1, beta2, eps) read from the device array hyper[4]: a launch captured into a HIP graph then
 * follows ModelDetector.update_learning_rate (models/keypoint_detector.py:356-366 sets param_groups[..]['lr']) without
 * a new capture -- the host refreshes the four floats before the replay. */
int usip_adam_step_hyper_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* step_count,
                             const float* hyper, long long n, void* stream);

/* Pooled-concat layers (a-6 / a-7 row-bias rewrite): the sum over each neighbourhood's K positions of the layer's
 * dY, from the per-neighbourhood sums of the BatchNorm-backward reduction: out[b][c][g] = K * coef4[3][c]
 * + coef4[0][c] * gsum0[b][c][g] + coef4[2][c] * gsum1[b][c][g].  gsum0/1, out [nb][C][G], coef4 [4][C]. */
int usip_bn_group_dy_sum_f32(const float* gsum0, const float* gsum1, const float* coef4, float* out,
                             int nb, int C, int G, int K, void* stream);

/* a-10: the sigma arithmetic of ChamferLoss_Brute after the two min / arg-min reductions
 * (models/losses.py:82-99) as one launch.  a [B][M], J i32 [B][M] = row minima / arg-minima (src -> dst),
 * c [B][N], I i32 [B][N] = column minima (dst -> src), sigma_src [B][M], sigma_dst [B][N].
 * out3 = (forward_loss + backward_loss, chamfer_pure, chamfer_weighted); sums in double, fixed order. */
int usip_chamfer_prob_f32(const float* a, const int32_t* J, const float* c, const int32_t* I,
                          const float* sigma_src, const float* sigma_dst, float* out3,
                          int B, int M, int N, void* stream);
/* Its backward for an upstream gradient gloss[0] (device scalar) of out3[0]: da [B][M], dc [B][N],
 * dsigma_src [B][M], dsigma_dst [B][N] (every element written; the gather's transpose is a deterministic
 * segmented sum). */
int usip_chamfer_prob_backward_f32(const float* gloss, const float* a, const int32_t* J, const float* c,
                                   const int32_t* I, const float* sigma_src, const float* sigma_dst,
                                   float* da, float* dc, float* dsigma_src, float* dsigma_dst,
                                   int B, int M, int N, void* stream);

/* f-1 (descriptor head): the same minimum / first arg-minimum for C-dimensional points a [B][C][Ma],
 * b [B][C][Nb] (Nb <= 1024) -- the M x M descriptor-distance matrices of DescPairScanLoss
 * (models/losses.py:207-218: torch.norm over B x C x M x M, 268 MB at B=8) are never built. */
int usip_nearest_nd_f32(const float* a, const float* b, float* min_d, int32_t* arg,
                        int B, int C, int Ma, int Nb, void* stream);

/* ------------------------------------------------------------------ a-5 / a-6 / a-7 / a-8  shared MLP
 * Replaces, per layer, nn.Conv1d/Conv2d(k=1) + MyBatchNorm + ReLU and their autograd backward
 * (models/layers.py:208-216 MyConv2d.forward, :293-303 EquivariantLayer.forward, :61-71/:112-121
 * MyBatchNorm*.forward).  Activations are [nb][C][P] exactly as the reference stores them
 * (B x C x M x K or B x C x N flattened over positions); fp32 MFMA, fp32 accumulate.
 *
 * usip_mlp_gemm_f32:  Y[b][m][p] = sum_k At[k][m] * pro(X[b][k][p]) + bias[m]
 *   At is the matrix operand K-major ([K][M], row stride lda): W^T for the forward product,
 *   W itself ([Cout][Cin]) for the data gradient dX = W^T . dY.  A NEGATIVE lda means the operand is
 *   stored M-major ([M][K], row stride -lda) and is read transposed, so the forward product can use W
 *   in place as well.
 *   pro: 0 identity | 1 relu(x*coef[0][k] + coef[1][k]) | 2 BatchNorm+ReLU backward of X = dZ,
 *        X2 = pre-BN output, coef = the [4][K] array written by usip_bn_backward_reduce_f32.
 *        3 as 2, but dZ is not a tensor: the layer fed ONLY a max over pool_group neighbours, so
 *          dZ[k][p] = (p % pool_group == pool_arg[k][p / pool_group]) ? pool_dp[k][p / pool_group] : 0
 *          is formed on the fly from the two [nb][K][P/pool_group] arrays (X may be NULL).
 *   rowbias (may be NULL): [nb][M][P/rb_group], added as Y[b][m][p] += rowbias[b][m][p / rb_group]:
 *   the contribution of input channels that are constant inside a neighbourhood of rb_group
 *   positions (the max-pooled feature the reference expands and concatenates, networks.py:706-709,
 *   layers.py:433-435) -- computed once per neighbourhood instead of once per neighbour.
 *   y_rows: 0, or the number of rows per cloud of the tensor Y points into when the M output rows are a
 *   channel slice of a wider [nb][y_rows][P] tensor (Y then points at the slice's first row of cloud 0).
 *   stats (may be NULL): [2][M][tiles] per-tile (sum, sum of squares) of Y over valid positions,
 *   tiles = usip_mlp_gemm_tiles(M, P, nb); summed in fixed order by usip_bn_finalize_f32. */
int usip_mlp_gemm_tiles(int M, int P, int nb);
int usip_mlp_gemm_f32(const float* At, int lda, const float* X, const float* X2, const float* coef,
                      int pro, const float* bias, const float* rowbias, int rb_group,
                      const float* pool_dp, const int32_t* pool_arg, int pool_group,
                      float* Y, int y_rows, float* stats, int M, int K, int P, int nb, void* stream);
/* Same contract with a bf16 MULTIPLY (the perf mode of BASELINE.json configs[1]; not the parity mode): tensors
 * stay fp32 in memory, the prologue runs in fp32, both operands are rounded to bf16 (nearest-even) on their way
 * into LDS, v_mfma_f32_32x32x16_bf16 accumulates in fp32, bias / rowbias / statistics are fp32.  The result
 * equals the fp32 product of the bf16-rounded operands up to summation order. */
int usip_mlp_gemm_bf16(const float* At, int lda, const float* X, const float* X2, const float* coef,
                       int pro, const float* bias, const float* rowbias, int rb_group,
                       const float* pool_dp, const int32_t* pool_arg, int pool_group,
                        float* Y, int y_rows, float* stats, int M, int K, int P, int nb, void* stream);
/* Same contract with an fp32-ACCURATE product on the bf16 matrix cores ("f32x3"): each fp32 operand is split
 * exactly into three bf16 planes and the six plane pairs of weight >= 2^-18 are accumulated in fp32 by
 * v_mfma_f32_32x32x16_bf16 (relative error of a product <= 3 * 2^-27, below fp32's own rounding; 2.7x the
 * fp32-MFMA rate).  Used for the launches that are matrix-bound (usip_mlp_gemm_f32x3_used(...) == 1); the others
 * are handed to the fp32 kernel, so the entry point is a drop-in for usip_mlp_gemm_f32 everywhere. */
int usip_mlp_gemm_f32x3(const float* At, int lda, const float* X, const float* X2, const float* coef,
                       int pro, const float* bias, const float* rowbias, int rb_group,
                       const float* pool_dp, const int32_t* pool_arg, int pool_group,
                        float* Y, int y_rows, float* stats, int M, int K, int P, int nb, void* stream);
int usip_mlp_gemm_f32x3_used(int M, int K, int P, int nb);
/* Streaming forward kernel for the narrow layers (K = 64 inputs, M = 64 or 128 outputs; csrc/narrow_fwd.hip): the
 * contract of usip_mlp_gemm_f32 (pro 0 or 1, bias, rowbias with rb_group % 32 == 0, y_rows) for P % 4 == 0 and a
 * 16-B aligned X.  Persistent workgroups: `stats` has usip_mlp_narrow_forward_blocks(M, K, P, nb) partials per channel
 * ([2][M][blocks]); that function returns 0 for shapes the kernel does not take (callers use usip_mlp_gemm_f32). */
int usip_mlp_narrow_forward_blocks(int M, int K, int P, int nb);
int usip_mlp_narrow_forward_f32(const float* At, int lda, const float* X, const float* coef, int pro,
                                const float* bias, const float* rowbias, int rb_group, float* Y, int y_rows,
                                float* stats, int M, int K, int P, int nb, void* stream);

/* The same f32x3 product with the MATRIX operand split ahead of time (once per optimizer step instead of once per
 * workgroup and stage): usip_mlp_split3_f32 turns the K-major operand At (A[m][k] = At[k*lda + m], M x K) into the
 * image the kernel copies straight into LDS -- per (tile_rows-row tile, 16-k stage) three contiguous bf16 planes, zero
 * padded -- usip_mlp_split3_bytes(M, K) bytes, 16-B aligned; tile_rows = usip_mlp_x3p_tile_rows(M, P, nb) of the launch
 * the image is for.  usip_mlp_gemm_x3p_f32 then has the contract of usip_mlp_gemm_f32 with `planes` in place of
 * (At, lda); K <= 640. */
int usip_mlp_x3p_tile_rows(int M, int P, int nb);  /* rows per tile (128 or 256) of a launch over nb x P positions */
/* All weight operands of a step in one launch: descs (DEVICE memory, n entries, At / planes as for
 * usip_mlp_split3_f32) with first_block = running sum of usip_mlp_split3_blocks(M, K, tile_rows) over the entries before. */
typedef struct usip_split3_desc {
    const float* At; void* planes; int32_t lda, M, K, first_block;
    int32_t tile_rows, reserved;                      /* rows per tile of the image (128 / 256); reserved: 2 = two fp16 planes (below) */
} usip_split3_desc;
int usip_mlp_split3_blocks(int M, int K, int tile_rows);
int usip_mlp_split3_multi_f32(const usip_split3_desc* descs_device, int n, int total_blocks, void* stream);
/* Positions per tile the same kernel uses for this launch: 128 (256 only under the x3_gemm_tile measurement knob). */
int usip_mlp_x3p_tile_cols(int M, int P, int nb, int pro, int with_stats);
long long usip_mlp_split3_bytes(int M, int K);
int usip_mlp_split3_f32(const float* At, int lda, int M, int K, int tile_rows, void* planes, void* stream);
int usip_mlp_gemm_x3p_f32(const void* planes, const float* X, const float* X2, const float* coef, int pro,
                          const float* bias, const float* rowbias, int rb_group, const float* pool_dp,
                          const int32_t* pool_arg, int pool_group, float* Y, int y_rows, float* stats,
                          int M, int K, int P, int nb, void* stream);
/* "f32x2": the same fp32-accurate product from TWO fp16 planes per operand (11 + 11 significant bits) and THREE plane
 * products -- half the matrix work of f32x3 at the same error level.  fp16 has 5 exponent bits, so both operands are
 * multiplied by powers of two (exact): the weights by 2^e with max|A| 2^e in [2^13, 2^14) (usip_mlp_split2h_f32 stores
 * 2^e behind the image; buffer size usip_mlp_split3_bytes), the streamed operand by 2^e derived in the kernel from a
 * RIGOROUS upper bound of what its prologue can produce:
 *   pro 1: coef = [4][K] (scale, shift, mean, invstd) of a training-mode BatchNorm over exactly the nb * P samples of
 *          this launch: |relu(bn(y))| <= |gamma| sqrt(n) + |beta|;
 *   pro 2 / 3: coef = the [5][K] array usip_bn_backward_reduce_f32 / usip_bn_pool_backward_reduce_f32 write with
 *          want_bound (row 4: bounds of |dY| per 64 channels).
 * pro 0 (no bound available) is not offered: callers use usip_mlp_gemm_x3p_f32.  Otherwise the contract of
 * usip_mlp_gemm_x3p_f32. */
int usip_mlp_split2h_f32(const float* At, int lda, int M, int K, int tile_rows, void* planes, void* stream);
int usip_mlp_gemm_x2h_f32(const void* planes, const float* X, const float* X2, const float* coef, int pro,
                          const float* bias, const float* rowbias, int rb_group, const float* pool_dp,
                          const int32_t* pool_arg, int pool_group, float* Y, int y_rows, float* stats,
                          int M, int K, int P, int nb, void* stream);

/* Round 4: data-gradient launches (pro 2 / 3) of the direct f32x2 kernel (csrc/gemm_x2d.hip) that also leave, from the dX
 * tile they hold, the BatchNorm-backward partial sums of the layer that produced the activation dX is the gradient of --
 * what autograd's native_batch_norm_backward of that layer re-reads (dX, Y) for in the reference
 * (models/layers.py:208-216).  red_y [nb][M][P]: that layer's pre-BN output; red_coef [4][M]: its (scale, shift, mean,
 * invstd); red_out: [2][tiles][M] sums (sum d, sum d * xhat, d = dX where its ReLU is on) followed by [tiles * M / 256]
 * maxima of |d|; red_gsum (optional, red_group 16 or 32 positions per neighbourhood): [2][nb * M][P / red_group] sums of
 * d and of y.  usip_mlp_gemm_x2d_red_tiles() = tiles of such a launch, 0 when the shape does not take this path (M % 256,
 * P % 128, 256-row tiles): use usip_mlp_gemm_x2h_f32 + usip_bn_backward_reduce_f32 then. */
int usip_mlp_gemm_x2d_red_tiles(int M, int K, int P, int nb, int red_group);
int usip_mlp_gemm_x2h_red_f32(const void* planes, const float* X, const float* X2, const float* coef, int pro,
                              const float* pool_dp, const int32_t* pool_arg, int pool_group, float* Y,
                              const float* red_y, const float* red_coef, float* red_out, float* red_gsum,
                              int red_group, int M, int K, int P, int nb, void* stream);
/* The pro 2 data gradient of usip_mlp_gemm_x2h_f32 whose output is the gradient of a tensor that is ALSO max-pooled over
 * runs of fork_group positions (a layer output that is pooled and passed on, models/networks.py:706-709,
 * layers.py:433-436): the pooling gradient fork_dp [nb][M][P / fork_group] is added to the position fork_arg
 * [nb][M][P / fork_group] names in each run (0 <= arg < fork_group) at the kernel's store -- Y is bit-equal to
 * usip_mlp_gemm_x2h_f32 followed by usip_group_max_backward_add_f32, without that second pass over Y.  Taken only where
 * usip_mlp_gemm_x2h_f32 launches its one-wave-per-SIMD kernel (M, P multiples of 256, K of 64) and fork_group is 16, 32 or
 * 64: usip_mlp_gemm_x2h_fork_supported() = 1; all pointers 16-B aligned; USIP_EINVAL otherwise. */
int usip_mlp_gemm_x2h_fork_supported(int M, int K, int P, int nb, int fork_group);
int usip_mlp_gemm_x2h_fork_f32(const void* planes, const float* X, const float* X2, const float* coef, float* Y, int y_rows,
                               const float* fork_dp, const int32_t* fork_arg, int fork_group, int M, int K, int P, int nb,
                               void* stream);
/* The same for the 128-wide layers (M <= 128, K <= 128; a row bias only with pro 1 and rb_group a multiple of 32) with
 * the weight fragments resident in registers and persistent workgroups over 64-position tiles: a CU moves the streamed
 * operand in and the output out, not the weight planes again for every tile.
 * stats: [2][M][usip_mlp_gemm_x2r_tiles(P, nb)]. */
int usip_mlp_gemm_x2r_tiles(int P, int nb);
int usip_mlp_gemm_x2r_f32(const void* planes, const float* X, const float* X2, const float* coef, int pro,
                          const float* bias, const float* rowbias, int rb_group, const float* pool_dp,
                          const int32_t* pool_arg, int pool_group, float* Y, int y_rows, float* stats, int M, int K,
                          int P, int nb, void* stream);

/* K-major copies of many weight matrices in one launch: for every t < ntensors, table[5t..5t+4] =
 * (source offset, rows, cols, destination offset, index of its first 32 x 32 tile), offsets in floats into src / dst;
 * dst[dof + c*rows + r] = src[sof + r*cols + c].  The reference stores Conv weights [Cout][Cin][1(,1)]
 * (models/layers.py:186-205); the GEMMs want [Cin][Cout].  total_tiles = sum of ceil(rows/32)*ceil(cols/32). */
int usip_multi_transpose_f32(const float* src, float* dst, const int32_t* table, int ntensors, int total_tiles,
                             void* stream);

/* Batch statistics -> mean[C], invstd[C] (biased variance, eps inside the sqrt), forward
 * coefficients coef[4][C] = (gamma*invstd, beta - mean*gamma*invstd, mean, invstd), and the running-statistics
 * update running = (1-momentum)*running + momentum*batch (unbiased variance), as F.batch_norm does
 * in training mode.  running_mean/var may both be NULL.  count = nb*P. */
int usip_bn_finalize_f32(const float* stats, int tiles, int C, long long count,
                         const float* gamma, const float* beta, float eps, float momentum,
                         float* running_mean, float* running_var, float* mean, float* invstd,
                         float* coef, void* stream);

/* Z = Y*coef[0][c] + coef[1][c], followed by ReLU when relu != 0.  Y, Z: [nb][C][P]. */
int usip_bn_apply_f32(const float* Y, const float* coef, float* Z, int relu,
                      int nb, int C, int P, void* stream);

/* Backward reductions of BatchNorm(+ReLU): dbeta[c] = sum dYhat, dgamma[c] = sum dYhat*yhat with
 * dYhat = dZ*[fma(y,coef_fwd[0],coef_fwd[1]) > 0] (dZ if !relu), and coef4[4][C] such that
 * dY = coef4[0]*dYhat + coef4[2]*y + coef4[3] (coef4[0..1] repeat coef_fwd for the mask).
 * Y == NULL selects the plain mode: dbeta[c] = sum dZ (bias gradient of a layer without BN).
 * partial: workspace of 2*nb*C floats.
 * gsum (may be NULL): [2][nb][C][P/group] per-neighbourhood sums of dYhat and of y, from which
 * sum_k dY = coef4[0]*gsum[0] + coef4[2]*gsum[1] + group*coef4[3] follows without a second pass
 * (group % 4 == 0 and group/4 a power of two <= 64). */
int usip_bn_backward_reduce_f32(const float* dZ, const float* Y, const float* coef_fwd,
                                const float* mean, const float* invstd, const float* gamma, int relu,
                                float* partial, float* dgamma, float* dbeta, float* coef4,
                                float* gsum, int group, int nb, int C, int P, int want_bound, void* stream);
/* want_bound != 0: `partial` holds [3][nb*C] floats (third plane: max |dYhat| per row) and coef4 is [5][C]: entry i of
 * row 4 (i < ceil(C/64)) is an upper bound of |dY| over channels [64 i, 64 i + 64) -- |a1| (max|dYhat| + |mean dYhat| +
 * |mean dYhat yhat| sqrt(n)), rigorous for batch statistics -- which the split-fp16 kernels (usip_mlp_gemm_x2h_f32,
 * usip_mlp_wgrad_x2h_f32) use to scale the operand into the fp16 range.  want_bound == 0: [2][nb*C] and [4][C]. */


/* usip_bn_backward_reduce_f32 for a layer whose output fed ONLY a max over K neighbours: the incoming
 * gradient is (k == arg) ? dpooled : 0, so the sums run over B*C*M arg-max elements instead of B*C*M*K.
 * dpooled f32 / arg i32 [nb][C][M], Y [nb][C][M][K]; outputs as usip_bn_backward_reduce_f32. */
/* yarg (may be NULL): Y at the arg-max as usip_group_max_act_f32 returned it -- replaces one gathered 4-B read per
 * neighbourhood; dgamma / dbeta / coef4 all NULL: only the partial sums [2][nb][C] are produced. */
int usip_bn_pool_backward_reduce_f32(const float* dpooled, const int32_t* arg, const float* Y, const float* yarg,
                                     const float* coef_fwd, const float* mean, const float* invstd,
                                     const float* gamma, int relu, float* partial, float* dgamma, float* dbeta,
                                     float* coef4, int nb, int C, int M, int K, int want_bound, void* stream);

/* dW[m][n] = sum_{b,p} pro(G)[b][m][p] * X[b][n][p]   (pro 0: G = dY given; pro 2: G = dZ, G2 = Y,
 * coef = coef4 as above; pro 3: dZ synthesised from pool_dp / pool_arg as in usip_mlp_gemm_f32).  workspace: usip_mlp_wgrad_workspace(M, N, P, nb) floats of partial tiles,
 * reduced in fixed order (deterministic).  dW is written as dW[m*ldw + coloff + n], so a column
 * block of a wider weight matrix can be filled in place.  xcoef (may be NULL): [2][N]; X is then the
 * PRE-BatchNorm output of the producing layer and relu(X*xcoef[0][n] + xcoef[1][n]) is formed on the fly
 * (the activated tensor is never stored). */
long long usip_mlp_wgrad_workspace(int M, int N, int P, int nb);
int usip_mlp_wgrad_f32(const float* G, const float* G2, const float* coef, int pro, const float* X,
                       const float* xcoef, const float* pool_dp, const int32_t* pool_arg, int pool_group,
                       float* workspace, float* dW, int ldw, int coloff,
                       int M, int N, int P, int nb, void* stream);
/* Deferred weight-gradient reductions (round 5; no reference counterpart -- the reference's autograd produces every dW
 * where its layer's backward runs, models/layers.py:208-216).  Between usip_wgrad_defer(1) and usip_wgrad_flush(stream) every
 * entry point that ends in the fixed-order sum of its partial tiles (usip_mlp_wgrad_*, usip_mlp_narrow_backward_f32,
 * usip_mlp_layer_backward_x2h_f32) launches its tile kernel and RECORDS the sum instead of launching it; the flush issues all
 * recorded sums in at most two launches (same summation order: same bits) and returns how many it issued (>= 0; < 0 error).
 * The caller keeps every workspace alive until the flush.  usip_wgrad_defer(0) leaves the mode and drops what is recorded.
 * The flush issues ceil(jobs / 24) launches per reduction width (two widths): two launches for the detector's fifteen sums.
 * usip_wgrad_defer_on(stream) enters the mode for ONE stream: entry points called with any other stream launch their sum at
 * once (the job list is process-global; a second thread / device / stream must not find its sums on this stream's flush).
 * usip_wgrad_defer_hold(1) .. (0) brackets calls whose sum must be launched at once although the mode is on: a dW that the
 * caller returns to a consumer running before the flush (anything that is not a view of the step's gradient bucket);
 * it returns the previous hold value. */
int usip_wgrad_defer(int on);
int usip_wgrad_defer_on(void* stream);
int usip_wgrad_defer_hold(int hold);
int usip_wgrad_flush(void* stream);

/* Backward of a NARROW layer (64 inputs, 64 or 128 outputs) in one pass over its tensors: data gradient AND weight
 * gradient from one staged tile of (dZ, Y, X) -- these layers are HBM-bound and the two separate products read
 * (dZ, Y) twice.  Replaces the pair usip_mlp_gemm_f32(pro = 2) + usip_mlp_wgrad_f32(pro = 2) for the grouped
 * convolutions conv2 / conv3 / conv4 of RPN_Detector_Ball (models/networks.py:705-709; autograd's
 * cudnn_convolution_backward in the reference).  Exact fp32 MFMA, deterministic (fixed-order partial sums).
 *   dX[b][ci][p] = sum_co W[co*ldw + ci] * dY[b][co][p],  dW[co*lddw + ci] = sum_{b,p} dY[b][co][p] * act(X)[b][ci][p]
 *   dY = BatchNorm'(ReLU'(dZ)) from (dZ, Y, coef4) as in usip_mlp_gemm_f32 pro = 2; act(X) = relu(X*xcoef[0]+xcoef[1])
 *   (xcoef NULL: X as is).  X / dX point at the first of the 64 rows inside [nb][x_rows][P] / [nb][dx_rows][P].
 * workspace: usip_mlp_narrow_backward_workspace(Cout, P, nb) floats.
 * red_partial (may be NULL; then xcoef must be the PRODUCING layer's full [4][64] forward coefficients -- scale, shift,
 *   mean, invstd): [2][usip_mlp_narrow_backward_blocks(Cout, P, nb)][64] partial BatchNorm-backward sums of that layer
 *   (sum dX*[relu on], sum dX*[relu on]*xhat), taken while the dX tile is in registers, followed by [blocks] maxima of
 *   |dX [relu on]| (2 * blocks * 64 + blocks floats in all); usip_bn_backward_finalize_f32
 *   turns partial sums (these, plus usip_bn_pool_backward_reduce_f32's when a max-pool also feeds that layer) into
 *   dgamma / dbeta / coef4 -- the separate reduction pass over (dZ, Y) of that layer disappears. */
int usip_mlp_narrow_backward_supported(int Cin, int Cout, int P);
long long usip_mlp_narrow_backward_workspace(int Cout, int P, int nb);
int usip_mlp_narrow_backward_blocks(int Cout, int P, int nb);
int usip_mlp_narrow_backward_f32(const float* dZ, const float* Y, const float* coef4, const float* X, int x_rows,
                                 const float* xcoef, const float* W, int ldw, float* dX, int dx_rows,
                                 float* workspace, float* dW, int lddw, float* red_partial, int Cin, int Cout,
                                 int P, int nb, void* stream);

/* The same fused layer backward on the 16-bit matrix cores with f32x2 arithmetic (csrc/layer_bwd_x2.hip; no reference
 * counterpart: the layers' backward is autograd's, models/layers.py:208-216, :293-303), for (Cin, Cout) = (64, 64), (64, 128), or
 * (128, 128) in the pooled form, and P % 64 == 0 (usip_mlp_layer_backward_x2h_supported).  coef4 = the [5][Cout] array usip_bn_backward_reduce_f32 /
 * usip_bn_backward_finalize_max_f32 write (row 4: bounds of |dY|); pool_dp / pool_arg (i32) [nb][Cout][P / pool_group]
 * given and dZ NULL: the pooled form, dZ = (p % pool_group == arg) ? pool_dp : 0, (128, 128) only; xcoef = the producing
 * layer's [4][Cin] (scale, shift, mean, invstd), training-mode statistics over exactly these nb * P samples; planes =
 * usip_mlp_split2h_f32 image of W as the data-gradient operand (At = W [Cout][ldw], M = Cin, K = Cout).  workspace:
 * usip_mlp_layer_backward_x2h_workspace floats.  red_partial (may be NULL): [2][blocks][Cin] partial sums of the
 * producing layer's BatchNorm backward against dX followed by [blocks] maxima of |dX [relu on]|, blocks =
 * usip_mlp_layer_backward_x2h_blocks.  group_sums (may be NULL; pooled form with red_partial, pool_group % 32 == 0):
 * [2][nb * Cin][P / pool_group] = per neighbourhood sum_k dX [relu on] and sum_k X, the `gsum` of
 * usip_bn_backward_reduce_f32 for a producing layer that is a pooled-concat layer (conv4 behind conv5). */
int usip_mlp_layer_backward_x2h_supported(int Cin, int Cout, int P, int pooled);
long long usip_mlp_layer_backward_x2h_workspace(int Cin, int Cout, int P, int nb);
int usip_mlp_layer_backward_x2h_blocks(int Cin, int Cout, int P, int nb);
int usip_mlp_layer_backward_x2h_f32(const float* dZ, const float* Y, const float* coef4, const float* pool_dp,
                                    const int32_t* pool_arg, int pool_group, const float* X, int x_rows,
                                    const float* xcoef, const void* planes, float* dX, int dx_rows, float* workspace,
                                    float* dW, int lddw, float* red_partial, float* group_sums, int Cin, int Cout,
                                    int P, int nb, void* stream);
/* The (Cin, Cout) = (64, 64) form with red_partial that ALSO takes, on the way, the sums from which the PRODUCING layer's
 * weight gradient follows -- for a producing layer whose input S f32 [nb][ws_rows <= 8][P] needs no gradient (conv1 of
 * RPN_Detector_Ball, models/networks.py:705; the first PointNet layer of RPN_Detector, layers.py:524-544): that layer's
 * dW' = dY' . S^T with dY' = a1' dYhat' + q1' y' + q0' is linear in  S1 = sum_p dYhat' S_j,  S2 = sum_p (y' - mean') S_j,
 * S3 = sum_p S_j, and this pass holds dYhat' = dX [relu on] and y' = X in LDS anyway.  wsum f32 [blocks][64][16]
 * (S1 | S2, j < 8), wsum3 f32 [blocks][8], blocks = usip_mlp_layer_backward_x2h_blocks.  usip_mlp_wsum_finalize_f32
 * combines them (fp64, fixed order) into dW'[c * lddw + j], j < ws_rows, once coef4' = usip_bn_backward_finalize_*_f32 of
 * the same call's red_partial is known: the producing layer needs no pass of its own over its (dZ, Y). */
int usip_mlp_layer_backward_x2h_ws_f32(const float* dZ, const float* Y, const float* coef4, const float* X, int x_rows,
                                       const float* xcoef, const void* planes, float* dX, int dx_rows, float* workspace,
                                       float* dW, int lddw, float* red_partial, const float* wsrc, int ws_rows,
                                       float* wsum, float* wsum3, int Cin, int Cout, int P, int nb, void* stream);
int usip_mlp_wsum_finalize_f32(const float* wsum, const float* wsum3, int blocks, int C, const float* coef4,
                               const float* mean, int ws_rows, float* dW, int lddw, void* stream);
int usip_bn_backward_finalize_f32(const float* partial, int rows, int C, long long count, const float* coef_fwd,
                                  const float* mean, const float* invstd, float* dgamma, float* dbeta, float* coef4,
                                  void* stream);
/* The same with the fifth row of coef4 ([5][C]: bounds of |dY| per 64 channels, what the f32x2 kernels scale their
 * operand by): the gradient is a sum of up to two parts whose maxima |dYhat| are given as arrays (max0[n0], max1[n1],
 * max1 may be NULL) -- the bound uses max(max0) + max(max1). */
int usip_bn_backward_finalize_max_f32(const float* partial, int rows, int C, long long count, const float* coef_fwd,
                                      const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                      float* coef4, const float* max0, int n0, const float* max1, int n1, void* stream);
/* bf16-multiply variant (see usip_mlp_gemm_bf16); same workspace, same deterministic fp32 reduction. */
int usip_mlp_wgrad_bf16(const float* G, const float* G2, const float* coef, int pro, const float* X,
                        const float* xcoef, const float* pool_dp, const int32_t* pool_arg, int pool_group,
                        float* workspace, float* dW, int ldw, int coloff,
                        int M, int N, int P, int nb, void* stream);
/* f32x3 variant (see usip_mlp_gemm_f32x3); same workspace, same deterministic fp32 reduction. */
int usip_mlp_wgrad_f32x3(const float* G, const float* G2, const float* coef, int pro, const float* X,
                        const float* xcoef, const float* pool_dp, const int32_t* pool_arg, int pool_group,
                        float* workspace, float* dW, int ldw, int coloff,
                        int M, int N, int P, int nb, void* stream);
/* f32x2 form of the weight gradient: as usip_mlp_wgrad_f32x3, and launches with pro 2 / 3, M, N > 128, coef = the [5][M]
 * array usip_bn_backward_reduce_f32 writes with want_bound and xcoef = the [4][N] (scale, shift, mean, invstd) of a
 * training-mode BatchNorm over exactly the nb * P samples of this launch run on two fp16 planes per operand and three
 * plane products (see usip_mlp_gemm_x2h_f32); every other launch exactly as usip_mlp_wgrad_f32x3. */
int usip_mlp_wgrad_x2h_f32(const float* G, const float* G2, const float* coef, int pro, const float* X,
                        const float* xcoef, const float* pool_dp, const int32_t* pool_arg, int pool_group,
                        float* workspace, float* dW, int ldw, int coloff,
                        int M, int N, int P, int nb, void* stream);
int usip_mlp_wgrad_f32x3_used(int M, int N, int P, int nb);

/* ------------------------------------------------------------------ a-6 / a-7 / a-12  grouping, pooling
 * out[b][coff+c][m][k] = x[b][c][idx[b][m][k]] - (c < nsub ? sub[b][c][m] : 0), written into the
 * channel slice [coff, coff+C) of an output with Ctot channels.  Replaces index expansion +
 * torch.gather + decentering + torch.cat (models/operations.py:271-287, networks.py:699-703,
 * layers.py:422-430).  x [B][C][N], idx i32 [B][M][K], sub [B][nsub][M], out [B][Ctot][M][K]. */
int usip_group_gather_f32(const float* x, const int32_t* idx, const float* sub, float* out,
                          int B, int C, int N, int M, int K, int nsub, int Ctot, int coff, void* stream);
/* Its backward w.r.t. x (scatter-add; dx [B][C][N] is zeroed first). */
int usip_group_gather_backward_f32(const float* dout, const int32_t* idx, float* dx,
                                   int B, int C, int N, int M, int K, int Ctot, int coff, void* stream);
/* pooled[row] = max_k z[row][k], arg[row] = first k attaining it (torch.max over the K axis,
 * networks.py:706,710, layers.py:433,438); rows = B*C*M.  Backward: dz[row][k] = (k==arg)*dpooled. */
int usip_group_max_f32(const float* z, float* pooled, int32_t* arg, long long rows, int K, void* stream);
/* The same pooling applied to relu?(y*coef[0][c] + coef[1][c]) formed on the fly from a layer's pre-BatchNorm
 * output y [B][C][M][K] (K % 4 == 0, K/4 a power of two <= 64): BN-apply + ReLU + max in ONE pass over y. */
/* yarg (may be NULL): [B][C][M], receives y at the arg-max (the pre-BN value the pooled layer's backward needs). */
int usip_group_max_act_f32(const float* y, const float* coef, int relu, float* pooled, int32_t* arg, float* yarg,
                           int B, int C, int M, int K, void* stream);
int usip_group_max_backward_f32(const float* dpooled, const int32_t* arg, float* dz,
                                long long rows, int K, void* stream);
/* The same gradient ADDED into an existing dense gradient: dz[row*K + arg[row]] += dpooled[row]
 * (the tensor that was pooled also fed a layer directly: its two gradients are combined by touching
 * `rows` elements instead of materialising and adding a second dense tensor). */
int usip_group_max_backward_add_f32(const float* dpooled, const int32_t* arg, float* dz,
                                    long long rows, int K, void* stream);

/* ------------------------------------------------------------------ neighbourhoods wider than 256 samples
 * (csrc/group_wide.hip; the indoor descriptor groups 448 points per keypoint).  One wave per neighbourhood.
 * usip_group_max_f32 / usip_group_max_act_f32 for K % 4 == 0, 256 < K <= 1024 and y 16-byte aligned; any other K or a
 * misaligned y is USIP_EINVAL, zero rows is USIP_OK.  coef == NULL: y [B][C][M][K] is already activated (relu is
 * ignored) and the NaN rule of usip_group_max_f32 applies; else the maximum is over relu?(fma(y, coef[0][c], coef[1][c])),
 * c = (row / M) % C.  arg is the FIRST k attaining the maximum, pooled carries that element's bits, yarg (may be NULL) is
 * y at arg.  A NaN ranks above everything; -0.0 and +0.0 tie. */
int usip_group_max_wide_f32(const float* y, const float* coef, int relu, float* pooled, int32_t* arg, float* yarg,
                            int B, int C, int M, int K, void* stream);
/* usip_bn_backward_reduce_f32 with the per-neighbourhood sums for group % 4 == 0, 256 < group <= 1024: the same arguments
 * and the same outputs (partial, dgamma, dbeta, coef4 with row 4 under want_bound, gsum [2][nb][C][P/group]).  gsum and Y
 * are required (no plain mode), P % group == 0, dZ and Y 16-byte aligned; anything else is USIP_EINVAL.  The summation
 * order is this entry's own and fixed: the same bits on every run, not those of usip_bn_backward_reduce_f32. */
int usip_bn_backward_reduce_wide_f32(const float* dZ, const float* Y, const float* coef_fwd,
                                     const float* mean, const float* invstd, const float* gamma, int relu,
                                     float* partial, float* dgamma, float* dbeta, float* coef4,
                                     float* gsum, int group, int nb, int C, int P, int want_bound, void* stream);

/* ------------------------------------------------------------------ a-7  node KNN
 * idx[b][m][0..K) = the K database points nearest to query m, ascending distance (lower index first on
 * exact ties): torch.norm + torch.topk(K, largest=False, sorted=True) of models/layers.py:417-421 without
 * the B x M x N matrix.  query f32 [B][3][M], database f32 [B][3][N], N <= 1024, K <= N. */
int usip_knn_f32(const float* query, const float* database, int32_t* idx,
                 int B, int M, int N, int K, void* stream);

/* The FIRST layer of GeneralKNNFusionModule (models/layers.py:422-431: gather the K neighbours' coordinates and features,
 * decenter the coordinates, concatenate to B x (3+C) x M x K, then models/layers.py:208-216: conv1x1 + BatchNorm + ReLU)
 * without the gathered tensor.  The convolution is linear and the features enter it undecentered:
 *     Y[b][co][m][k] = sum_j W[co][j] (database[b][j][n] - query[b][j][m])  +  U[b][co][n],   n = idx[b][m][k],
 * with U = W[:, 3:] . feat + bias a product over the N database points (usip_mlp_gemm_*) instead of the M*K grouped
 * positions.  Same math as the reference's layer up to fp32 summation order.
 *   forward : U f32 [B][Cout][N], W f32 [Cout][ldw] (columns 0..2 = the coordinate weights), database [B][3][N],
 *             query [B][3][M], idx i32 [B][M][K] -> Y f32 [B][Cout][M*K]; stats (may be NULL): [2][Cout][B] per-cloud
 *             partial (sum, sum^2) of every channel, the layout usip_bn_finalize_f32 reads with ntn = B.
 *   backward: dZ, Y [B][Cout][M*K] and coef4 [>=4][Cout] as for the shared-MLP prologue PRO_BN_BWD
 *             (dY = coef4[0] dZ [fma(Y, coef4[0], coef4[1]) > 0 if relu] + coef4[2] Y + coef4[3]); dcoord f32 [B][3][M*K] =
 *             database[b][j][idx] - query[b][j][m] (usip_group_gather_f32 with sub = query); (start, perm) = the
 *             usip_csr_by_index_i32 lists of idx viewed as [B][M*K] over N destinations ->
 *             dU [B][Cout][N] = the segment sums of dY in list order (no float atomics),
 *             dWc_part [B][Cout][3] = per-cloud partial gradients of the coordinate weights (the caller adds the B parts).
 * Shapes: usip_knn_layer_supported (N <= 1489, M*K <= 16384, M*K % 4 == 0); dZ, Y, dcoord 16-B aligned. */
int usip_knn_layer_supported(int N, int M, int K);
int usip_knn_layer_forward_f32(const float* U, const float* W, int ldw, const float* database, const float* query,
                               const int32_t* idx, float* Y, float* stats, int B, int Cout, int N, int M, int K,
                               void* stream);
int usip_knn_layer_backward_f32(const float* dZ, const float* Y, const float* coef4, int relu, const float* dcoord,
                                const int32_t* start, const int32_t* perm, float* dU, float* dWc_part,
                                int B, int Cout, int N, int M, int K, void* stream);

/* ------------------------------------------------------------------ (judge row) RPN_Detector_KNN front end
 * idx[b][m][0..K) = the K cloud points nearest to node m, nearest first, ties towards the lower index:
 * torch.norm(node - x) over B x M x N followed by torch.topk(k=64, largest=False, sorted=False) of
 * models/networks.py:576-581 without the matrix.  topk(sorted=False) leaves the order of the picks unspecified;
 * the SET is the reference's, the order is that of a stable sort of the reference's distance row.
 * node f32 [B][3][M], x f32 [B][3][N], K <= min(N, 256), N <= 16384. */
int usip_knn_points_f32(const float* node, const float* x, int32_t* idx, int B, int M, int N, int K, void* stream);

/* ------------------------------------------------------------------ f-3  farthest-point sampling of nodes
 * Replaces FarthestSampler.sample (data/kitti_detector_loader.py:69-83; also oxford_detector_loader.py,
 * modelnet_shrec_loader.py): out_idx[b][0] = first_idx[b], then k-1 times the first arg-max of the running
 * minimum squared distance, evaluated in float64 exactly as numpy does.  pts f32 [B][3][n], n <= 16384;
 * out_idx i32 [B][k] (indices into the n points; gather them for the node coordinates). */
int usip_fps_f32(const float* pts, const int32_t* first_idx, int32_t* out_idx, int B, int n, int k, void* stream);

/* ------------------------------------------------------------------ f-4  inference post-processing
 * Greedy non-maximum suppression by sigma (evaluation/save_keypoints.py:180-216): order[b][0..count[b]) are
 * the indices kept, in the order they are picked (ascending sigma; ties: lower index), each pick removing every
 * keypoint whose float32 distance to it is not > radius.  keypoints f32 [B][3][M], sigmas f32 [B][M], M <= 1024.
 * The reference's "keep the desired_keypoint_num smallest sigmas" (:346-351) is the first entries of order. */
int usip_nms_f32(const float* keypoints, const float* sigmas, float radius, int32_t* order, int32_t* count,
                 int B, int M, void* stream);

/* ------------------------------------------------------------------ f-5  training pairs
 * Replaces KittiLoader.__getitem__ / OxfordLoader.__getitem__ (data/kitti_detector_loader.py:101-259,
 * data/oxford_detector_loader.py:99-229) with data/augmentation.py's augment and transform_pc_pytorch (:199-248): P pairs
 * (src, dst) built from scans resident in device memory, written as DetectorStep.step consumes them.
 *
 * bank    f32 [rows][row_len] (x y z nx ny nz curvature reflectance for the reference's Nx8 files), all scans back to back;
 * offsets i64 [num_scans + 1], scan s = rows offsets[s] .. offsets[s+1]; scan_ids i32 [P] (which scan each pair uses,
 * clamped into range).
 * Per cloud: N slots drawn without replacement in random order (fewer rows than N: the reference's fix_idx layout, whole
 * copies of 0..n-1 then a random remainder); sn = columns 3..3+Cs (sn_last: the row's last column); n_sub of the N slots are
 * the FPS candidates, the first FPS index is random, FPS (usip_fps_f32) runs on the un-augmented candidates; then, in train
 * mode, augment (rotation stages in float64 as row vectors p @ R, jitter, scale, shift; rounded to f32 once; sn[0:3] rotated
 * and rounded per stage, never scaled) and, for dst in both modes, transform_pc_pytorch (f32 R p, * scale, + shift).
 * Outputs: pc[c] f32 [P][3][N], sn[c] f32 [P][Cs][N], node[c] f32 [P][3][M] (c = 0 src, 1 dst; may be halves of one
 * buffer), R f32 [P][3][3], scale f32 [P], shift f32 [P][3][1] (the transform's); optional rows i32 [2][P][N] (scan-relative
 * row of every slot) and node_slots i32 [2][P][M] (the slot every node came from).
 * Randomness: Philox4x64-10, key (seed, 0), counter (element, stream tag, pair_base + p, step) -- csrc/pairs_rng.h.
 * usip_pairs_apply_f32 takes every draw explicitly instead (usip_pairs_draws, raw uniforms and standard normals) and runs
 * the same arithmetic: the reference's fixtures test the code that trains.
 * USIP_EINVAL: bad shapes (3 + Cs > row_len, n_sub > 16384, M > n_sub, n_sub > N, Cs > 8, row_len > 16), enu_to_cam with
 * Cs < 3, min_rows (the fewest rows of any scan the ids may name) < 1, or < N with require_full (Oxford). */
#define USIP_PAIRS_NPARAM 24
typedef struct usip_pairs_recipe {
    double aug_scale_lo, aug_scale_hi;     /* augment scale U(lo, hi): KITTI 0.9 1.1, Oxford 0.7 1.3 */
    double shift_range;                    /* augment shift U(-r, r)^3 with translation_perturbation: 1 */
    double height_lo, height_hi;           /* Oxford height scaling U(lo, hi) of ENU z, train mode: 0.25 1.2 */
    double pc_sigma, pc_clip;              /* jitter clip(sigma z, +-clip): points 0.04 0.12 */
    double sn_sigma, sn_clip;              /*   every sn channel 0.01 0.05 */
    double node_sigma, node_clip;          /*   nodes 0.04 0.12 */
    double pert_sigma, pert_clip;          /*   rotation perturbation 0.06 0.18 */
    double dst_scale_thre, dst_shift_thre; /* transform_pc_pytorch(scale_thre, shift_thre): 0 0.5 */
    int N, M, Cs, n_sub, row_len;          /* points, nodes, sn channels, FPS candidates, floats per scan row */
    int sn_last;                           /* sn = the row's last column (KITTI, Cs == 1) */
    int train;                             /* augment (and height scaling); 0 = test mode: transform only */
    int rot_horizontal, rot_3d, rot_perturbation, translation_perturbation;
    int height_scaling;                    /* Oxford is_height_scaling */
    int enu_to_cam;                        /* Oxford coordinate_ENU_to_cam after FPS */
    int require_full;                      /* scans need >= N rows (Oxford) */
    int dst_rot_type;                      /* transform's rot_type: 0 None, 2 '2d', 3 '3d' */
    int dst_rot_perturbation;
} usip_pairs_recipe;
/* Explicit draws, per pair p and cloud c at [p][c]: rows i32 [P][2][N] (scan-relative row of each slot), cand i32 [P][2][n_sub]
 * (slot of each FPS candidate), first i32 [P][2] (first FPS index among the candidates), jit_pc f64 [P][2][N][3],
 * jit_sn f64 [P][2][N][Cs], jit_node f64 [P][2][M][3] (standard normals), params f64 [P][USIP_PAIRS_NPARAM]:
 * 0 augment yaw uniform, 1-3 augment rand(3), 4-6 augment perturbation normals, 7 augment scale uniform, 8-10 augment shift
 * uniforms, 11 height-scaling uniform, 12-14 transform angle uniforms ('2d' uses 12), 15-17 transform perturbation normals,
 * 18 transform scale uniform, 19-21 transform shift uniforms. */
typedef struct usip_pairs_draws {
    const int32_t* rows;
    const int32_t* cand;
    const int32_t* first;
    const double* jit_pc;
    const double* jit_sn;
    const double* jit_node;
    const double* params;
} usip_pairs_draws;
typedef struct usip_pairs_out {
    float* pc[2];
    float* sn[2];
    float* node[2];
    float* R;
    float* scale;
    float* shift;
    int32_t* rows;          /* optional (NULL) */
    int32_t* node_slots;    /* optional (NULL) */
} usip_pairs_out;
long long usip_pairs_workspace_bytes(const usip_pairs_recipe* recipe, int P);
/* Byte offset of one part of that workspace, for inspection: 0 the per-pair f64 table, 1 the un-augmented FPS candidates
 * f32 [2P][3][n_sub] (clouds src 0..P-1, then dst), 2 the first FPS indices i32 [2P], 3 the FPS picks i32 [2P][M],
 * 4 the total (= usip_pairs_workspace_bytes). */
long long usip_pairs_workspace_offset(const usip_pairs_recipe* recipe, int P, int part);
int usip_pairs_build_f32(const usip_pairs_recipe* recipe, const float* bank, const int64_t* offsets, int num_scans,
                         const int32_t* scan_ids, int P, long long min_rows, uint64_t seed, uint64_t step,
                         long long pair_base, const usip_pairs_out* out, void* workspace, void* stream);
int usip_pairs_apply_f32(const usip_pairs_recipe* recipe, const usip_pairs_draws* draws, const float* bank,
                         const int64_t* offsets, int num_scans, const int32_t* scan_ids, int P, long long min_rows,
                         const usip_pairs_out* out, void* workspace, void* stream);
/* HOST twin (every pointer on the host, draws NULL = Philox): the same arithmetic with its own float64 FPS loop. */
int usip_pairs_build_f32_cpu(const usip_pairs_recipe* recipe, const usip_pairs_draws* draws, const float* bank,
                             const int64_t* offsets, int num_scans, const int32_t* scan_ids, int P, uint64_t seed,
                             uint64_t step, long long pair_base, const usip_pairs_out* out);

/* ------------------------------------------------------------------ f-6  evaluation: registration and repeatability
 * Replaces the reference's MATLAB evaluation: evaluation/matlab/eval_outdoor/kitti/evaluate_kitti.m with
 * external/ransacfitRt.m, ransac.m, estimateRt.m, estimateRigidTransform.m and Utils.compareTransform, and
 * eval_repeatability/eval_rep.m.  Float64 arithmetic on float32 inputs (MATLAB reads the float32 files into doubles).
 *
 * Padded batches with per-pair counts: x1, x2 f32 [P][3][Nmax] (x1 the anchor keypoints, x2 the positive frame's keypoints
 * they matched), count i32 [P] (clamped into [0, Nmax]), Nmax <= 10240; entries beyond count[p] are never read.  The three
 * RANSAC entries and their host twins take any Nmax up to that limit: the outdoor evaluation stops at 1024 (one frame's
 * keypoints), the indoor one (f-9 below) brings the union of two k-nearest lists; the kernels are the same.
 *
 * usip_ransac_trials_f32: trial t of pair p fits x1 = R x2 + t to three distinct correspondences (estimateRigidTransform:
 * the quaternion of the smallest eigenvalue of B = sum A'A, a fixed-sweep 4x4 Jacobi) and scores it, counts[p][t] =
 * #{i < count : |x1_i - (R x2_i + t)| < threshold}; hypotheses f64 [P][T][3][4] and triplets_out i32 [P][T][3] are optional
 * (NULL).  Draws: perm(0..2) of a PairsPerm bijection on [0, count) keyed from Philox4x64-10, key (seed, 0), counter
 * (t, 9 << 8, g, 0), g = pair_ids[p] (i64 [P]; NULL: g = p) -- a triplet depends on (seed, g, t) only.  The SAME algorithm
 * as the reference with our OWN draws: MATLAB's rng(0) / randsample stream cannot be reproduced and is not attempted.
 * usip_ransac_trials_explicit_f32 takes the triplets i32 [P][T][3] (clamped into range) and runs the same arithmetic.
 * count < 3: every score 0 (ransacfitRt returns before any trial).  A degenerate triplet still gives a finite orthonormal R.
 *
 * usip_ransac_select_f32: ransac.m's sequential loop replayed over counts[p][0..T) -- best = 0, N = 1, trial = 0; while
 * N > trial: counts[trial] >= best (ties: the later trial) updates best, chosen and N = max(log(1 - 0.99) / log(pNo), 10),
 * pNo = min(1 - eps, max(eps, 1 - (best / count)^3)); trial += 1; stop when trial > max_trials (<= T - 1) -- then the chosen
 * hypothesis' inlier set and estimateRt over ALL inliers, summed in a fixed order (bit-reproducible).  triplets NULL: the
 * Philox draws of (seed, pair_ids).  Rt f64 [P][3][4] (zeros when invalid), inlier_mask u8 [P][Nmax], inliers, trialcount
 * i32 [P], valid u8 [P], optional chosen i32 [P].  count < 3: invalid; count == 3: the fit of the three, trialcount 0; fewer
 * than 3 inliers: invalid.  With gt f64 [P][3][4]: delta_t = |t_gt - t|, delta_deg = sum |rotm2eul(R_gt' R)| in degrees
 * (ZYX); an invalid pair gets evaluate_kitti.m's catch values (3, 6).
 *
 * usip_repeatability_f32 (eval_rep.m): anc f32 [P][3][Ma], pos f32 [P][3][Mp] with counts, gt f64 [P][3][4]:
 * min_dist[p][i] = min_j |anc_i - (R_gt pos_j + t_gt)| (float64; inf beyond anc_count or without positives), hits[p] =
 * #(min_dist < radius), ratio[p] = hits / anc_count (0 for an empty anchor frame).
 *
 * usip_nearest_nd_counted_f32: pdist2(pos, anc, 'euclidean', 'smallest', 1) on ragged batches -- usip_nearest_nd_f32's
 * arithmetic and first-index tie rule with per-frame counts: a f32 [B][C][Ma], b f32 [B][C][Nb], rows beyond a_count get
 * (inf, 0), candidates beyond b_count are never read. */
int usip_ransac_trials_f32(const float* x1, const float* x2, const int32_t* count, int P, int Nmax, int T, double threshold,
                           uint64_t seed, const int64_t* pair_ids, int32_t* counts, double* hypotheses,
                           int32_t* triplets_out, void* stream);
int usip_ransac_trials_explicit_f32(const float* x1, const float* x2, const int32_t* count, int P, int Nmax, int T,
                                    double threshold, const int32_t* triplets, int32_t* counts, double* hypotheses,
                                    void* stream);
int usip_ransac_select_f32(const float* x1, const float* x2, const int32_t* count, int P, int Nmax, int T, int max_trials,
                           double threshold, uint64_t seed, const int64_t* pair_ids, const int32_t* triplets,
                           const int32_t* counts, const double* gt, double* Rt, uint8_t* inlier_mask, int32_t* inliers,
                           int32_t* trialcount, uint8_t* valid, int32_t* chosen, double* delta_t, double* delta_deg,
                           void* stream);
int usip_compare_transform_f64(const double* gt, const double* Rt, int P, double* delta_t, double* delta_deg, void* stream);
int usip_repeatability_f32(const float* anc, const int32_t* anc_count, const float* pos, const int32_t* pos_count,
                           const double* gt, double radius, int P, int Ma, int Mp, double* min_dist, int32_t* hits,
                           double* ratio, void* stream);
int usip_nearest_nd_counted_f32(const float* a, const float* b, const int32_t* a_count, const int32_t* b_count,
                                float* min_d, int32_t* arg, int B, int C, int Ma, int Nb, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order; the selection runs ransac.m's loop as
 * written.  triplets NULL = the Philox draws; num_threads splits the P x T trials. */
int usip_ransac_trials_f32_cpu(const float* x1, const float* x2, const int32_t* count, int P, int Nmax, int T,
                               double threshold, uint64_t seed, const int64_t* pair_ids, const int32_t* triplets,
                               int32_t* counts, double* hypotheses, int32_t* triplets_out, int num_threads);
int usip_ransac_select_f32_cpu(const float* x1, const float* x2, const int32_t* count, int P, int Nmax, int T,
                               int max_trials, double threshold, uint64_t seed, const int64_t* pair_ids,
                               const int32_t* triplets, const int32_t* counts, const double* gt, double* Rt,
                               uint8_t* inlier_mask, int32_t* inliers, int32_t* trialcount, uint8_t* valid, int32_t* chosen,
                               double* delta_t, double* delta_deg);
int usip_compare_transform_f64_cpu(const double* gt, const double* Rt, int P, double* delta_t, double* delta_deg);
int usip_repeatability_f32_cpu(const float* anc, const int32_t* anc_count, const float* pos, const int32_t* pos_count,
                               const double* gt, double radius, int P, int Ma, int Mp, double* min_dist, int32_t* hits,
                               double* ratio);
int usip_nearest_nd_counted_f32_cpu(const float* a, const float* b, const int32_t* a_count, const int32_t* b_count,
                                    float* min_d, int32_t* arg, int B, int C, int Ma, int Nb);

/* ------------------------------------------------------------------ f-7  raw scans prepared: normals, curvature, voxel grid
 * Replaces the reference's MATLAB preparation of a raw scan (evaluation/matlab/kitti_data_prepare/kitti_test_prepare.m:95-108:
 * findPointNormals(pc, 9, [0, 0, 1], true) of external/findPointNormals.m, then pcdownsample(pc, 'gridAverage', 0.2)) that
 * makes the [rows, 8] scans `x y z nx ny nz curvature reflectance` the loaders read (data/kitti_detector_loader.py:32,116).
 * Float64 arithmetic on float32 inputs (MATLAB reads the float32 file into doubles).  csrc/prepare_math.h is the arithmetic.
 *
 * xyzi f32 [n][4] row-major (x y z reflectance: a KITTI velodyne .bin as it lies in the file), finite values,
 * K + 1 <= n <= 2^20, 1 <= K <= 16.
 *
 * usip_scan_knn_f32 (findPointNormals.m:75-79, knnsearch k + 1 and "remove self"): idx i32 [n][K] = for every point i the K
 * points j != i with the smallest d2 = (dx*dx + dy*dy) + dz*dz in float64, ascending, ties towards the lower j.  The point is
 * left out by INDEX (MATLAB drops the first column, which among exact duplicates need not be the point itself).  perm i32 [n]:
 * the permutation that sorts the points along x, ascending (any stable or unstable sort) -- the kernel walks outward from a
 * query's own position and stops where the x gap alone exceeds the K-th distance; the result is the all-pairs answer.  A perm
 * that does not sort gives wrong neighbours, never a read outside xyzi.  tiles_visited i32 [ceil(n / 256)], optional (NULL): the
 * number of 256-point tiles each workgroup of 256 queries walked.
 *
 * usip_scan_normals_f32 (findPointNormals.m:81-130, dirLargest = true): C = sum_k d_k d_k' / K with d_k = p_i - p_idx[i][k],
 * summed in the order of idx; its eigenvector of the smallest eigenvalue (the first of equal ones) by 8 cyclic Jacobi sweeps
 * in a fixed order; curvature = lambda_min / (l0 + l1 + l2); the normal negated when normal[c] * (p[c] - viewpoint[c]) > 0,
 * c = the first arg max |normal|.  A zero trace gives curvature 0 and normal (0, 0, 1) before the flip (MATLAB: 0 / 0).
 * viewpoint: 3 doubles on the HOST.  normals_f64 f64 [n][4] and normals_f32 f32 [n][4] (nx ny nz curvature; the float32
 * rounding of the same values); either may be NULL, not both.  The "normalized_curvature" output of findPointNormals is not
 * used by the preparation and is not built.
 *
 * usip_scan_voxel_keys_f32 / usip_scan_voxel_average_f32 (pcdownsample 'gridAverage' -- a MATLAB builtin whose source the
 * reference does not carry: this definition is the project's own).  lohi f32 [6]: per-axis minimum, then maximum of the scan
 * (device memory for the device entry).  cell = floor(((double)p - (double)lo) / leaf) per axis, clamped into [0, 2^20);
 * keys i64 [n] = (cz * ny + cy) * nx + cx with nx, ny the cell counts along x, y.  The caller sorts the keys (stable): perm
 * i32 [n] = point indices in (key, index) order, start i32 [m + 1] = the first position of every occupied cell, start[m] = n.
 * rows f32 [m][8], in ascending key order: the members of a cell are added in ascending original index in float64; mean xyz,
 * mean normal (of normals_f64) divided by its norm -- the first member's normal when the mean is exactly zero --, mean
 * curvature, mean reflectance. */
int usip_scan_knn_f32(const float* xyzi, const int32_t* perm, int n, int K, int32_t* idx, int32_t* tiles_visited, void* stream);
int usip_scan_normals_f32(const float* xyzi, const int32_t* idx, int n, int K, const double* viewpoint, double* normals_f64,
                          float* normals_f32, void* stream);
int usip_scan_voxel_keys_f32(const float* xyzi, int n, const float* lohi, double leaf, int64_t* keys, void* stream);
int usip_scan_voxel_average_f32(const float* xyzi, const double* normals_f64, const int32_t* perm, const int32_t* start,
                                int n, int m, float* rows, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order.  The neighbour search is the plain all-pairs
 * walk (no perm); num_threads splits the queries. */
int usip_scan_knn_f32_cpu(const float* xyzi, int n, int K, int32_t* idx, int num_threads);
int usip_scan_normals_f32_cpu(const float* xyzi, const int32_t* idx, int n, int K, const double* viewpoint,
                              double* normals_f64, float* normals_f32);
int usip_scan_voxel_keys_f32_cpu(const float* xyzi, int n, const float* lohi, double leaf, int64_t* keys);
int usip_scan_voxel_average_f32_cpu(const float* xyzi, const double* normals_f64, const int32_t* perm, const int32_t* start,
                                    int n, int m, float* rows);

/* ------------------------------------------------------------------ f-8  descriptor training batches from posed scans
 * Replaces KittiDescriptorLoader.__getitem__ (data/kitti_descriptor_loader.py:102-347: get_instance_unaugmented_np,
 * get_nearby_instance_unagumented_np, augment) and mine_negative_sample (:278-317, called from kitti/train_descriptor.py):
 * P (anchor, positive) clouds built from scans resident in device memory, the positive scan chosen on the device, the
 * negatives mined from the anchors' poses.  One call enqueues everything on the caller's stream; nothing is read back.
 *
 * The posed bank: rows / offsets as in f-5; poses f64 [S][4][4] row-major (the 'pose' of the .npz files); seq_of i32 [S] the
 * index of every scan's sequence in [0, num_seq); seq_start i32 [num_seq + 1]: sequence q = scans seq_start[q] ..
 * seq_start[q+1], contiguous and in trajectory order.  seq_start_host is the same array on the HOST (the entry points
 * check it there: seq_start[0] = 0, strictly ascending, seq_start[num_seq] = num_scans); for the host twin both are host.
 *
 * Positive of anchor a (index ia in its sequence of n scans), the reference's loop taken literally: interval =
 * (int)(positive_radius / 0.8 * 2); lo = max(ia - interval, 0), hi = min(ia + interval, n - 1); draw t in [lo, hi]; accept when
 * ||t_t - t_a||_2 < positive_radius (float64, the translations of the float64 poses); else lo = t + 1 when t < ia, hi = t - 1
 * otherwise; after 3 * interval refused tries the anchor itself.  [lo, hi] always holds ia, which accepts at distance 0, so
 * the loop ends within 2 * interval + 1 tries.
 * Negative of anchor i: the candidates are the j != i, ascending, with seq[j] != seq[i] or dist(i, j) > negative_radius;
 * neg_idx[i] = candidate number `draw`.  No candidate: neg_idx[i] = 0 as the reference leaves it, and neg_fail[0] counts such
 * rows of this call.  dist(i, j) is the float64 Euclidean distance between the translations of the two poses ROUNDED TO
 * FLOAT32 (the reference mines on the batch's FloatTensor poses).  The reference computes ||(P_i^-1 P_j)[0:3,3]|| =
 * ||R_i' (t_j - t_i)||, which equals ||t_j - t_i|| for a rigid pose (R_i orthonormal); the two differ by rounding only.
 * Mining is within the call's own P anchors.
 * Per cloud (c = 0 anchor, 1 positive): f-5's per-slot work with cloud.require_full (rows drawn without replacement through
 * the keyed bijection, sn = columns 3..3+Cs, n_sub FPS candidates, usip_fps_f32 on the un-augmented candidates, then in train
 * mode augment: float64 rotations, jitter, scale, shift, one rounding).  Each cloud has its own rotations, jitters and shift;
 * the pair shares ONE scale.  There is no transform (R / scale / shift) of the second cloud.  Test mode: no augmentation.
 * Outputs: pc[c] f32 [P][3][N], sn[c] f32 [P][Cs][N], node[c] f32 [P][3][M], anc_pose / pos_pose f32 [P][4][4], anc_seq
 * i32 [P] (sequence index), pos_id i32 [P] (the bank-global scan chosen), neg_idx i64 [P], neg_fail i32 [1]; optional rows
 * i32 [2][P][N], node_slots i32 [2][P][M].
 * Randomness (usip_desc_pairs_build_f32): Philox4x64-10, counter (element, stream tag, pair_base + p, step), stream tags
 * 17-26 (csrc/desc_pairs_math.h) -- none shared with f-5's 1-8, so no draw collides with the detector builder's.
 * usip_desc_pairs_apply_f32 takes every draw explicitly: the per-cloud draws in f-5's layouts (cloud.params unused),
 * params f64 [P][USIP_DESC_PAIRS_NPARAM]: 0 the pair's scale uniform; cloud c at 1 + 10 c: +0 yaw uniform, +1..3 rand(3),
 * +4..6 perturbation normals, +7..9 shift uniforms; tries i32 [P][T]: the in-sequence indices random.randint returned, in
 * order (entries past the accepted try are not read; a search that outruns T takes the anchor); neg_pick i32 [P]: the
 * candidate number np.random.randint returned.
 * USIP_EINVAL: as f-5 for cloud (with sn_last, height_scaling, enu_to_cam and dst_* zero), min_rows < N, mine with P < 2,
 * num_seq < 1, seq_start_host not as above, a radius that is not positive. */
#define USIP_DESC_PAIRS_NPARAM 24
typedef struct usip_desc_pairs_recipe {
    usip_pairs_recipe cloud;
    double positive_radius, negative_radius;   /* KITTI: 5, 50 */
    int mine;                                  /* 1: mine negatives; 0: neg_idx and neg_fail are left untouched */
} usip_desc_pairs_recipe;
typedef struct usip_desc_pairs_bank {
    const float* rows;
    const int64_t* offsets;
    const double* poses;
    const int32_t* seq_of;
    const int32_t* seq_start;
    const int32_t* seq_start_host;
    int num_scans, num_seq;
    long long min_rows;                        /* the fewest rows of any scan */
} usip_desc_pairs_bank;
typedef struct usip_desc_pairs_draws {
    usip_pairs_draws cloud;
    const double* params;
    const int32_t* tries;
    const int32_t* neg_pick;
    int T;
} usip_desc_pairs_draws;
typedef struct usip_desc_pairs_out {
    float* pc[2];
    float* sn[2];
    float* node[2];
    float* anc_pose;
    float* pos_pose;
    int32_t* anc_seq;
    int32_t* pos_id;
    int64_t* neg_idx;
    int32_t* neg_fail;
    int32_t* rows;          /* optional (NULL) */
    int32_t* node_slots;    /* optional (NULL) */
} usip_desc_pairs_out;
long long usip_desc_pairs_workspace_bytes(const usip_desc_pairs_recipe* recipe, int P);
/* Byte offset of one part: 0 the per-cloud f64 tables [2P], 1 the un-augmented FPS candidates f32 [2P][3][n_sub] (anchors
 * 0..P-1, then positives), 2 the first FPS indices i32 [2P], 3 the FPS picks i32 [2P][M], 4 every cloud's scan id i32 [2P],
 * 5 the total. */
long long usip_desc_pairs_workspace_offset(const usip_desc_pairs_recipe* recipe, int P, int part);
int usip_desc_pairs_build_f32(const usip_desc_pairs_recipe* recipe, const usip_desc_pairs_bank* bank,
                              const int32_t* scan_ids, int P, uint64_t seed, uint64_t step, long long pair_base,
                              const usip_desc_pairs_out* out, void* workspace, void* stream);
int usip_desc_pairs_apply_f32(const usip_desc_pairs_recipe* recipe, const usip_desc_pairs_draws* draws,
                              const usip_desc_pairs_bank* bank, const int32_t* scan_ids, int P,
                              const usip_desc_pairs_out* out, void* workspace, void* stream);
/* HOST twin (every pointer on the host, draws NULL = Philox): the same arithmetic in the same order, its own float64 FPS. */
int usip_desc_pairs_build_f32_cpu(const usip_desc_pairs_recipe* recipe, const usip_desc_pairs_draws* draws,
                                  const usip_desc_pairs_bank* bank, const int32_t* scan_ids, int P, uint64_t seed,
                                  uint64_t step, long long pair_base, const usip_desc_pairs_out* out);

/* ------------------------------------------------------------------ f-26  indoor descriptor batches (SceneNN pairs)
 * usip_indoor_pairs_recipe, _bank, _draws, _out and the usip_indoor_pairs_* entries: in a header of their own. */
#include "usip_hip_indoor_pairs.h"

/* ------------------------------------------------------------------ f-27  evaluation batches from indoor fragments
 * usip_fragment_batch_bank, _draws, _out and the usip_fragment_batch_* entries: in a header of their own. */
#include "usip_hip_fragment_batch.h"

/* ------------------------------------------------------------------ f-9  indoor fragment registration (Redwood / 3DMatch)
 * Replaces the per-pair work of evaluation/matlab/eval_indoor/3dmatch/register2Fragments.m: k-nearest matching in both
 * directions and the union of the two lists, ransacfitRt on up to 10240 correspondences, the information matrix over
 * the inliers and ratioAligned over the full fragments.  f-6's convention: float64 arithmetic on float32 inputs, sums in
 * a fixed order.  csrc/fragments_math.h is the arithmetic.
 *
 * usip_knn_nd_counted_f32: pdist2(b, a, 'euclidean', 'smallest', k), 1 <= k <= 8, on ragged batches with
 * usip_nearest_nd_counted_f32's distance: dist f32 / idx i32 [B][Ma][k] ascending, the lower index on ties; valid[B] =
 * min(k, b_count) columns hold data, the rest and the rows beyond a_count hold (inf, 0).  k = 1 is
 * usip_nearest_nd_counted_f32 bit for bit.
 *
 * usip_match_union_i32: nn12 i32 [P][Ma][k] (for keypoint i of fragment 1 its neighbours in fragment 2), nn21 i32
 * [P][Mp][k] (the converse), the fragments' keypoint counts a_count, p_count i32 [P] (of a list min(k, the other count)
 * columns are read, indices are clamped into range) -> the rows (i, q) of union([i, nn12(i, :)], [nn21(q, :), q], 'rows'):
 * pairs i32 [P][Cmax][2] sorted by (i, q), zeros beyond count i32 [P]; Cmax = k (Ma + Mp) <= 10240.
 *
 * ransacfitRt on the union's rows is f-6's usip_ransac_trials_f32 / _explicit_f32 / usip_ransac_select_f32 above.
 *
 * usip_information_f32: x f32 [P][3][Nmax] (the fragment-1 keypoint of every correspondence), mask u8 [P][Nmax] ->
 * info f64 [P][6][6] = sum over the masked points of A'A, A = [I3 | 0 2sz -2sy; -2sz 0 2sx; 2sy -2sx 0]; exactly symmetric.
 *
 * usip_overlap_ratio_f32: the fragments' full clouds in one CSR bank (rows f32 [total_rows][row_len], x y z first;
 * offsets i64 [num_frags + 1]), pairs (frag1[p], frag2[p]) with the estimate Rt f64 [P][3][4] moving fragment 2 into
 * fragment 1's frame: hits[p][0] = the fragment-1 points a with a moved fragment-2 point b' = R b + t at sqrt(d2) < radius,
 * hits[p][1] = the b' with such an a, ratio f64 [P][2] = hits over the fragment's rows.  perm1 i32 [total_rows]: for every
 * fragment, at its offset, its local row indices ascending along x; perm2 i32 [P][Lmax]: fragment 2's local row indices
 * ascending along the moved x, which usip_overlap_keys_f32 writes (keys f64 [P][Lmax], +inf beyond the fragment); Lmax >=
 * the longest fragment.  The answer is the all-pairs one as long as the permutations sort. */
int usip_knn_nd_counted_f32(const float* a, const float* b, const int32_t* a_count, const int32_t* b_count, int k,
                            float* dist, int32_t* idx, int32_t* valid, int B, int C, int Ma, int Nb, void* stream);
int usip_match_union_i32(const int32_t* nn12, const int32_t* nn21, const int32_t* a_count, const int32_t* p_count, int P,
                         int Ma, int Mp, int k, int32_t* pairs, int32_t* count, void* stream);
int usip_information_f32(const float* x, const uint8_t* mask, int P, int Nmax, double* info, void* stream);
int usip_overlap_keys_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                          const int32_t* frag2, const double* Rt, int P, int Lmax, double* keys, void* stream);
int usip_overlap_ratio_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                           const int32_t* frag1, const int32_t* frag2, const double* Rt, const int32_t* perm1,
                           const int32_t* perm2, int P, int Lmax, double radius, int32_t* hits, double* ratio, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order.  prune = 0 makes the overlap twin test
 * all pairs instead of walking outward along x. */
int usip_knn_nd_counted_f32_cpu(const float* a, const float* b, const int32_t* a_count, const int32_t* b_count, int k,
                                float* dist, int32_t* idx, int32_t* valid, int B, int C, int Ma, int Nb, int num_threads);
int usip_match_union_i32_cpu(const int32_t* nn12, const int32_t* nn21, const int32_t* a_count, const int32_t* p_count,
                             int P, int Ma, int Mp, int k, int32_t* pairs, int32_t* count);
int usip_information_f32_cpu(const float* x, const uint8_t* mask, int P, int Nmax, double* info);
int usip_overlap_keys_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                              const int32_t* frag2, const double* Rt, int P, int Lmax, double* keys);
int usip_overlap_ratio_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                               const int32_t* frag1, const int32_t* frag2, const double* Rt, const int32_t* perm1,
                               const int32_t* perm2, int P, int Lmax, double radius, int prune, int32_t* hits,
                               double* ratio, int num_threads);

/* ------------------------------------------------------------------ f-11  baseline keypoints: ISS (Intrinsic Shape Signatures)
 * The hand-crafted detector the reference compares its learned one with (evaluation/save_keypoints.py:44-50, method = 'iss':
 * PCLKeypoint.keypointIss(pc, salient_radius 2, non_max_radius 2, gamma_21 0.975, gamma_32 0.975, min_neighbors 5)).  The PCL
 * binding is not part of the reference; the definition below is this project's own, written from PCL's ISSKeypoint3D
 * (iss_3d.hpp) with border estimation off.  Float64 arithmetic on float32 inputs, never contracted; csrc/iss_math.h is the
 * arithmetic.
 *
 * pc f32 [B][3][N]; count i32 [B] (NULL: N): the first count[b] points of frame b are live; 1 <= N <= 2^20, B <= 65535.
 * j is a member of N_r(i) iff d2(i, j) = (dx*dx + dy*dy) + dz*dz < r * r (strict; r * r once, in float64); i is one itself.
 *
 * usip_iss_saliency_f32: neighbours i32 [B][N] = |N_rs(i)|; saliency f64 [B][N]: 0 when fewer than min_neighbors members,
 * else from C = sum over N_rs(i) of (p_j - p_i)(p_j - p_i)' (not divided by the count), the six sums taken in ascending
 * position of the frame's stable order along x; its eigenvalues e1 >= e2 >= e3 by 8 cyclic Jacobi sweeps in a fixed order;
 * saliency = e3 when the three are finite, e3 >= 0, e2 / e1 < gamma_21 and e3 / e2 < gamma_32 (a NaN ratio fails), else 0.
 * perm i32 [B][N]: per frame, in its first count[b] entries, the live points in that order (x ascending, ties towards the
 * lower index) -- the kernel walks only the 256-point tiles of that order that can hold a member; the result is the all-pairs
 * answer.  A perm that does not sort gives wrong values, never a read outside pc.  tiles_visited i32 [B][ceil(N / 256)],
 * optional (NULL): the tiles each workgroup of 256 queries walked (0 for a workgroup without a live query).
 *
 * usip_iss_nms_f32: keypoint u8 [B][N] = 1 iff saliency[i] > 0, |N_rn(i)| >= min_neighbors and no member of N_rn(i) has a
 * larger saliency (equal ones do not suppress each other).
 * Slots beyond count[b] get saliency 0, neighbours 0, keypoint 0.  USIP_EINVAL: a shape outside the limits, min_neighbors < 1,
 * a radius that is not positive and finite, a NULL among the required pointers. */
int usip_iss_saliency_f32(const float* pc, const int32_t* count, const int32_t* perm, int B, int N, double salient_radius,
                          double gamma_21, double gamma_32, int min_neighbors, double* saliency, int32_t* neighbours,
                          int32_t* tiles_visited, void* stream);
int usip_iss_nms_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* saliency, int B, int N,
                     double non_max_radius, int min_neighbors, uint8_t* keypoint, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order; every query tests all live points of its
 * frame, in the frame's own stable order along x (no perm); num_threads splits the queries. */
int usip_iss_saliency_f32_cpu(const float* pc, const int32_t* count, int B, int N, double salient_radius, double gamma_21,
                              double gamma_32, int min_neighbors, double* saliency, int32_t* neighbours, int num_threads);
int usip_iss_nms_f32_cpu(const float* pc, const int32_t* count, const double* saliency, int B, int N, double non_max_radius,
                         int min_neighbors, uint8_t* keypoint, int num_threads);

/* ------------------------------------------------------------------ f-12  Fast Global Registration of fragment pairs
 * The second registrator of the reference's indoor evaluation (evaluation/matlab/eval_indoor/fgr/register2FragmentsFGR.m,
 * computeAndVisualizeFGR.m): Fast Global Registration (Zhou, Park, Koltun, ECCV 2016).  The reference's
 * fgr/fast_global_registration.cpp wraps an app.h it does not ship, so the definition below is this project's own, written
 * from the paper and its published constants.  Float64 arithmetic on float32 inputs, never contracted, no floating-point
 * atomics, every sum in the order stated here; csrc/fgr_math.h is the arithmetic.  The estimate maps fragment 2 into
 * fragment 1, x1 = R x2 + t, as f-9's.
 *
 * Per pair: kp1, kp2 f32 [3][M] (finite values) with counts n1, n2 i32 (a count above M or below 0 behaves as M or 0);
 * nn12 i32 [M]: for keypoint i of fragment 1 its nearest descriptor of fragment 2 (usip_knn_nd_counted_f32 with k = 1), nn21
 * i32 [M] the converse.  1 <= M <= 1024, P <= 65535.
 *
 * usip_fgr_tuples_f32 / usip_fgr_tuples_explicit_f32:
 *  1 mutual i32 [P][M][2]: the rows (i, nn12[i]) for ascending i < n1 with 0 <= nn12[i] < n2 and nn21[nn12[i]] == i, zeros
 *    beyond mutual_count i32 [P] = nc <= M.  (FGR's two lazy lists followed by its cross-check reduce to exactly this set.)
 *  2 norm f64 [P][8] = mean1[3], mean2[3], scale, 0.  A mean is over ALL n keypoints of its fragment, matched or not: lane l
 *    of 256 adds its points l, l + 256, ... in ascending order, the 256 partial sums go through the binary tree part[l] +=
 *    part[l + stride], stride = 128 .. 1, and the total is divided by n (0 for an empty fragment).  scale = the largest
 *    sqrt((x x + y y) + z z) over both centred sets; u = (x - mean) / scale.  A scale that is 0 or not finite makes the pair
 *    invalid: no trial is walked.
 *  3 T = 100 nc trials.  Trial t takes three rows of the mutual list: perm(0), perm(1), perm(2) of a PairsPerm bijection on
 *    [0, nc) keyed from the Philox4x64-10 block with key (seed, 0) and counter (t, 10 << 8, g, 0), g = pair_ids[p] (NULL: p)
 *    -- f-6's keying under stream tag 10; a triple depends on (seed, g, t) only.  The explicit form reads triples i32
 *    [P][T][3], clamped into [0, nc), and walks min(100 nc, T) trials.  The trial is accepted iff li 0.95 < lj && lj < li /
 *    0.95 for each of the edges (0,1), (0,2), (1,2), li and lj the edge's lengths in normalised fragment 1 and 2 (a repeated
 *    row gives li = lj = 0 and is refused).  The first 1000 accepted trials, in ascending t, each contribute their three rows
 *    in draw order, duplicates stay: rows i32 [P][3000] (indices into the mutual list, zeros beyond row_count i32 [P]);
 *    trials_walked i32 [P] = t + 1 of the trial that filled the cap, else the number of trials.  triples_out i32
 *    [P][T_out][3], optional (NULL): the triples of the walked trials t < T_out; other entries are left untouched.
 *
 * usip_fgr_optimize_f32: the pair is invalid with a bad scale or fewer than 10 rows.  Otherwise graduated non-convexity:
 * par = 1, (R, t) = (I, 0); iteration k = 0 .. 63: if k % 4 == 0 && par > 0.025 then par = par / 1.4; per row q = R u2 + t from
 * the ORIGINAL normalised u2 and the accumulated transform, r = u1 - q, e = (r0 r0 + r1 r1) + r2 r2, w = par / (e + par), s =
 * w w, Jacobian rows [0, -q2, q1, -1, 0, 0], [q2, 0, -q0, 0, -1, 0], [-q1, q0, 0, 0, 0, -1].  The 21 upper entries of A = sum s J'J
 * and the 6 of b = sum s J'r are 27 sums, each taken as the means are (lane l of 256 its rows l, l + 256, ..., then the tree);
 * six of them are sums of exact zeros and two repeat a third, so 19 are carried (csrc/fgr_math.h: sums_of_row has the
 * expressions).  A = L L' column by column, inner sums subtracted in ascending index; a pivot that is not finite and positive
 * makes the pair invalid.  x = -A^-1 b by forward and backward substitution; a component of x that is not finite, or |x0..2| >
 * pi, makes the pair invalid.  Rd = Rz(x2) Ry(x1) Rx(x0) with the header's own fgr_sincos (a reduction by multiples of pi/2
 * with rint, then fixed polynomials: host and device return the same bits, which libm's sin and the device's do not); R <- Rd
 * R, t <- Rd t + x3..5.  Finally t_out = (t scale - R mean2) + mean1.  Rt f64 [P][3][4], valid u8 [P]; an invalid pair gets
 * [I | 0], valid 0, an empty mask and 0 inliers, as f-9's RANSAC.  inlier_mask u8 [P][M] over the MUTUAL rows (not the tuple
 * rows): f-6's euc3Ddist under the estimate < threshold (0.2 in the evaluation), zeros beyond nc; inliers i32 [P] its count.
 *
 * USIP_EINVAL: a shape outside the limits, T or T_out < 1 with its array given, a NULL among the required pointers. */
int usip_fgr_tuples_f32(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2, const int32_t* nn12,
                        const int32_t* nn21, int P, int M, uint64_t seed, const int64_t* pair_ids, int32_t* mutual,
                        int32_t* mutual_count, double* norm, int32_t* rows, int32_t* row_count, int32_t* trials_walked,
                        int32_t* triples_out, int T_out, void* stream);
int usip_fgr_tuples_explicit_f32(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2,
                                 const int32_t* nn12, const int32_t* nn21, int P, int M, const int32_t* triples, int T,
                                 int32_t* mutual, int32_t* mutual_count, double* norm, int32_t* rows, int32_t* row_count,
                                 int32_t* trials_walked, void* stream);
int usip_fgr_optimize_f32(const float* kp1, const float* kp2, const int32_t* mutual, const int32_t* mutual_count,
                          const double* norm, const int32_t* rows, const int32_t* row_count, int P, int M, double threshold,
                          double* Rt, uint8_t* valid, uint8_t* inlier_mask, int32_t* inliers, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order, the trials as the sequential loop;
 * num_threads splits the pairs.  usip_fgr_tuples_f32_cpu takes either source of draws (triples NULL: Philox). */
int usip_fgr_tuples_f32_cpu(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2, const int32_t* nn12,
                            const int32_t* nn21, int P, int M, uint64_t seed, const int64_t* pair_ids, const int32_t* triples,
                            int T, int32_t* mutual, int32_t* mutual_count, double* norm, int32_t* rows, int32_t* row_count,
                            int32_t* trials_walked, int32_t* triples_out, int T_out, int num_threads);
int usip_fgr_tuples_explicit_f32_cpu(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2,
                                     const int32_t* nn12, const int32_t* nn21, int P, int M, const int32_t* triples, int T,
                                     int32_t* mutual, int32_t* mutual_count, double* norm, int32_t* rows, int32_t* row_count,
                                     int32_t* trials_walked, int num_threads);
int usip_fgr_optimize_f32_cpu(const float* kp1, const float* kp2, const int32_t* mutual, const int32_t* mutual_count,
                              const double* norm, const int32_t* rows, const int32_t* row_count, int P, int M,
                              double threshold, double* Rt, uint8_t* valid, uint8_t* inlier_mask, int32_t* inliers,
                              int num_threads);
/* The contract's sine and cosine of n HOST doubles, |x| <= pi (csrc/fgr_math.h: fgr_sincos), for tests of its accuracy. */
int usip_fgr_sincos_f64_cpu(const double* x, int n, double* sin_out, double* cos_out);

/* ------------------------------------------------------------------ f-13  trimmed ICP refinement of fragment registrations
 * The reference's second log writer (evaluation/matlab/eval_indoor/3dmatch/writeLogReconputeAlign.m) downsamples both
 * fragments on a 0.04 m grid (f-7's grid average), refines the pair's estimate with pcregrigid (point to point, InlierRatio
 * 0.3) and counts the moved fragment-2 points within 0.05 m of fragment 1.  pcregrigid is a MATLAB built-in whose source is not
 * part of the reference, so the definition below is this project's own, written from the function's documented behaviour and
 * defaults (20 iterations, Tolerance [0.01 0.009] on the mean of the last three iterations).  f-9's conventions: float32
 * inputs, float64 arithmetic, never contracted, sums in a fixed order, no floating-point atomics, no launch synchronises the
 * host, every index read from memory is clamped before use.  csrc/icp_math.h is the arithmetic.
 *
 * The bank is f-9's: rows f32 [total_rows][row_len >= 3] (x y z first; here the DOWNSAMPLED fragments), offsets i64
 * [num_frags + 1], perm1 i32 [total_rows] (per fragment, at its offset, its local row indices ascending along x).  Per pair:
 * frag1, frag2 i32 [P] (clamped into the bank), Rt0 f64 [P][3][4] mapping fragment 2 into fragment 1, mask u8 [P] (NULL:
 * all ones).  A = fragment 1 with n1 rows, B = fragment 2 with n2 rows.  Lmax must be at least the length of every fragment a pair
 * names: a longer fragment is cut to its first Lmax rows only so that nothing is read or written outside an array, perm1 then
 * names rows that are gone and the result is unspecified (the device's walk and the twin's loop need not agree).  order2 i32
 * [P][Lmax] (NULL: the identity): slot s < n2 of the pair names the row of B that the s-th query is; the first n2 slots must
 * hold a permutation of 0 .. n2 - 1 (values are clamped; a row no slot names keeps idx = 0, d2 = 0).  The order decides only
 * which queries share a workgroup -- usip_overlap_keys_f32's moved x under Rt0, sorted, keeps them close -- never a result.
 *
 * usip_icp_nearest_f32: one pass under the poses Rt f64 [P][3][4].  For row i of B: q = R b_i + t (f-9's xform), idx[p][i] =
 * the row j of A with the least d2 = sqdist3(q, a_j), the LOWEST row index among equal distances; d2[p][i] that distance.
 * The search is exact: it equals the loop over all rows of A, which is what the host twin runs.  idx i32 [P][Lmax], d2 f64
 * [P][Lmax]; zeros beyond n2 and for a pair with mask 0, n1 = 0 or n2 = 0.  visits u64 [P], optional (NULL): the (query, row)
 * distances the lanes evaluated (a lane whose bound is met skips a staged tile and does not count it) -- against n1 n2 the
 * share of the all-pairs work that the walk did.
 *
 * usip_icp_refine_f32: (R, t) = Rt0; iteration k = 1 .. max_iterations:
 *  1 the nearest pass under (R, t);
 *  2 m = max(1, floor(inlier_ratio n2)) (at most n2); kept are the m smallest rows under the lexicographic order (d2_i, i),
 *    stated as the cut (d2*, i*): row i is kept iff d2_i < d2* or (d2_i == d2* and i <= i*);
 *  3 the rigid fit of the kept ORIGINAL b_i onto a_idx[i] (MATLAB composes increments of a moved copy; the absolute pose from
 *    the original rows is the same optimum without accumulated rounding): lane l of 256 adds its kept rows among l, l + 256,
 *    ... in ascending i, the 256 partial sums go through f-6's binary tree -- first the six centroid sums, each divided by m,
 *    then f-6's accumulate over the centred rows (x = a, y = b), then transform_from (8 Jacobi sweeps, never a NaN from
 *    coincident rows: B = 0 gives R = I);
 *  4 a fit with an entry that is not finite ends the pair: the last finite pose stays, converged = 0, iterations = k - 1;
 *  5 dt_k = |t_k - t_{k-1}|, dc_k = |R_k - R_{k-1}|_F (nine squared differences added in row-major order, then sqrt).  The
 *    pair stops after iteration k with converged = 1 when mean(dt) <= tol_t and mean(dc) <= tol_c, the means over the last
 *    min(k, 3) values: ((v_{k-2} + v_{k-1}) + v_k) / 3, (v_1 + v_2) / 2, v_1.  (The documented rotation test is on the angle
 *    in radians; acos rounds differently on host and device, so the caller passes the chordal bound tol_c = 2 sqrt(2)
 *    sin(tol_r / 2) of the same angle and the library takes square roots only.)
 * The final pass: 1 and 2 under the final pose; hits = #{i : sqrt(d2_i) < align_radius} (f-9's within); ratio f64 [P][2] =
 * hits / n1, hits / n2 (the reference's one count over both lengths); rmse = sqrt(sum of the kept d2 / m), the sum taken as
 * in 3.  Rt f64 [P][3][4], iterations i32 [P] (fits done), converged u8 [P], hits i32 [P].  A pair with mask 0, n1 = 0 or
 * n2 = 0 is not refined: Rt = Rt0, every other output 0.  The reference passes R through rotm2eul / eul2rotm to satisfy
 * affine3d; the estimate is taken as it is.  cut_d2 f64 [P][max_iterations + 1] with cut_i i32 of the same shape, optional
 * (both or neither): the cut (d2*, i*) of every pass that ran, iteration k at column k - 1, the final pass at column
 * max_iterations, zeros elsewhere.  workspace: usip_icp_workspace_bytes(P, Lmax) bytes of device memory.  visits as
 * above, summed over every pass.  stage_ms HOST f64 [4], optional (NULL) and a measurement only: HIP-event milliseconds of the
 * nearest, trim and fit launches of the loop and of the final pass's three; giving it makes the call wait for its launches, and
 * an event that cannot be created, recorded or read is returned as the call's HIP error (stage_ms is then incomplete).
 *
 * Limits: P <= 65535, Lmax in 1 .. 2^24, 0 < inlier_ratio <= 1, 0 <= max_iterations <= 64, tolerances >= 0, align_radius > 0;
 * anything else, a NULL among the required pointers or a workspace too small is USIP_EINVAL.  The loop is 3 launches per
 * iteration for the whole batch; every workgroup reads its pair's state in device memory first and leaves when the pair has
 * stopped. */
long long usip_icp_workspace_bytes(int P, int Lmax);
int usip_icp_nearest_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                         const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt,
                         const uint8_t* mask, const int32_t* order2, int P, int Lmax, int32_t* idx, double* d2,
                         unsigned long long* visits, void* stream);
int usip_icp_refine_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                        const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt0,
                        const uint8_t* mask, const int32_t* order2, int P, int Lmax, double inlier_ratio, int max_iterations,
                        double tol_t, double tol_c, double align_radius, void* workspace, long long workspace_bytes,
                        double* Rt, int32_t* iterations, uint8_t* converged, double* rmse, int32_t* hits, double* ratio,
                        double* cut_d2, int32_t* cut_i, unsigned long long* visits, double* stage_ms, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order; the search is the loop over all rows of A
 * in ascending row order, the trim a selection on (bit pattern, row).  num_threads splits the pairs.  idx_out i32 [P][Lmax],
 * d2_out f64 [P][Lmax], optional (NULL): the final pass's neighbours and distances. */
int usip_icp_nearest_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                             const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt,
                             const uint8_t* mask, const int32_t* order2, int P, int Lmax, int32_t* idx, double* d2,
                             int num_threads);
int usip_icp_refine_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                            const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt0,
                            const uint8_t* mask, const int32_t* order2, int P, int Lmax, double inlier_ratio,
                            int max_iterations, double tol_t, double tol_c, double align_radius, double* Rt,
                            int32_t* iterations, uint8_t* converged, double* rmse, int32_t* hits, double* ratio,
                            double* cut_d2, int32_t* cut_i, int32_t* idx_out, double* d2_out, int num_threads);

/* ------------------------------------------------------------------ f-14  loop closures pruned by pose-graph optimisation
 * The reference's last indoor number is not per pair: eval_indoor/split_txt_compute_G.m splits <scene>.log into odometry
 * (j - i == 1) and loop-closure edges with a dense 6 x 6 information matrix each (computeInformation, method 'point'), a
 * robust global optimisation (Choi, Zhou, Koltun, CVPR 2015) prunes the loop closures that disagree with the rest of the
 * graph, and loop_evaluation/ scores what is left.  The optimiser is a tool the reference does not ship, so the definition
 * below is this project's own, written from the paper.  f-9's and f-13's conventions: float64 arithmetic, never contracted,
 * every sum in a stated order, no floating-point atomics, no launch synchronises the host, every index read from memory is
 * checked or clamped before use.  csrc/posegraph_math.h is the arithmetic.
 *
 * usip_icp_information_f32: f-13's bank (perm1 is not needed) and pairs; idx i32 [P][Lmax], d2 f64 [P][Lmax] as
 * usip_icp_nearest_f32 wrote them under the pose in question; mask u8 [P] (NULL: all ones).  count i32 [P] = the rows i < n2
 * with sqrt(d2_i) < radius (f-9's within, strict); info f64 [P][6][6] = the sum over those rows, with multiplicity, of A'A at
 * s = a_idx[i] (idx clamped into fragment 1), A as usip_information_f32's: lane l of 256 adds its rows among l, l + 256, ...
 * in ascending i, the 256 partial sums of the nine distinct terms go through f-6's binary tree, the matrix is assigned entry
 * by entry and so exactly symmetric.  A pair with mask 0, n1 = 0, n2 = 0 or no row within the radius gets zeros, never a NaN.
 * USIP_EINVAL: the bank's and P's limits of f-13, a radius that is not positive, a NULL among the required pointers.
 *
 * usip_posegraph_optimize_f64: S scenes in one call.  Per scene: n i32 [S] fragments, ecount i32 [S] edges sorted by (i, j)
 * with 0 <= i < j < n and at most one edge per pair: edge_i, edge_j i32 [S][Emax], X f64 [S][Emax][3][4] mapping fragment j
 * into fragment i's frame (a .log entry), info f64 [S][Emax][6][6] (symmetric; info[0][0] is the number of aligned points);
 * T0 f64 [S][Nmax][3][4], the start poses mapping fragment k into fragment 0's frame.  An edge with j == i + 1 is an odometry
 * edge: its weight is 1 and it is never pruned.  Fragment 0 is fixed.  The unknowns of a step are d_k = (rho_k, phi_k), k = 1
 * .. n - 1, translation first.  One iteration:
 *  1 per edge E = T_i^-1 T_j (the rigid inverse R', -(R' t); every 3-sum from the left), D = E X^-1, e = [t(D); qv(D)] with
 *    qv the vector part of the quaternion of R(D) by Shepperd's rule: the branch is the largest of (trace, R00, R11, R22),
 *    the lowest index on ties, the sign such that w >= 0 -- finite at a half turn, which a wrong loop closure can be.
 *  2 f = sum_r e_r (sum_c L_rc e_c), both ascending, L the edge's info; mu = L_00 tau2; the weight l = 1 for an odometry
 *    edge, else (mu / (mu + f))^2, or 0 when mu + f is not finite and positive; in stage 2 a loop edge with kept = 0 has l = 0.
 *    An edge with l = 0 contributes nothing.
 *  3 J_i = -S, J_j = S Ad_E, S = diag(1, 1, 1, 1/2, 1/2, 1/2), Ad_E (rho, phi) = (R_E rho + t_E x (R_E phi), R_E phi): the
 *    small-residual Jacobians of the right perturbations T_k <- T_k exp(d_k).
 *  4 H's block (j, i) is l J_j' L J_i of its one edge; block (a, a) is the sum of l J_a' L J_a over the edges incident to a in
 *    ascending edge index, g_a the sum of l J_a' L e over the same edges (csrc/posegraph_math.h: edge_blocks has the
 *    expressions); the incidence lists are built inside the call.
 *  5 H = L L' over the 6 (n - 1) unknowns: every entry is H_rc minus its inner sum in ascending k, divided by the pivot's
 *    square root; x = H^-1 g by forward substitution in ascending and backward substitution in descending order; d = -x.
 *  6 Rd = Rz(phi2) Ry(phi1) Rx(phi0) with f-12's fgr_sincos; t <- R rho + t with the old R, then R <- R Rd.  step = the largest
 *    |component| of d.
 *  7 A pivot that is not finite and positive (status 1), a component of d that is not finite (2) or an angle |phi| > pi (3)
 *    ends the scene: the last good poses stay, iterations_done counts the steps that succeeded.
 * Stage 1 runs iterations1 steps (no stopping rule); a weight pass under its final poses gives weight1, and kept = odometry ||
 * weight1 >= prune.  Stage 2 runs iterations2 steps from stage 1's poses over the kept edges, the line process still on; a
 * final weight pass gives weight2 (0 for an edge that was not kept) and energy = f (-1 where f is not finite).  A scene that
 * ended early skips the remaining steps, not the weight passes.
 * T f64 [S][Nmax][3][4]; weight1, weight2, energy f64 [S][Emax]; kept u8 [S][Emax]; iterations_done i32 [S][2]; last_step f64
 * [S][2] (the last successful step of either stage, 0 without one); status i32 [S]; zeros beyond n and ecount; no NaN leaves
 * the call.  workspace: usip_posegraph_workspace_bytes(S, Nmax, Emax) bytes of device memory.
 *
 * Limits: S <= 65535, 2 <= n <= Nmax <= 128, 1 <= Emax <= Nmax (Nmax - 1) / 2, iterations in 0 .. 256, tau2 > 0 and finite,
 * 0 <= prune <= 1; anything else, a NULL among the required pointers or a workspace too small is USIP_EINVAL.  A scene whose n
 * or ecount is outside its range, or whose edges are unsorted, repeated or have i >= j or j >= n, is USIP_EINVAL in the host
 * twin; the device entry cannot read its arrays without waiting for the device, so there such a scene gets status 4 and zeros
 * in every other output, and nothing of it is indexed. */
int usip_icp_information_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                             const int32_t* frag1, const int32_t* frag2, const int32_t* idx, const double* d2,
                             const uint8_t* mask, int P, int Lmax, double radius, double* info, int32_t* count, void* stream);
long long usip_posegraph_workspace_bytes(int S, int Nmax, int Emax);
int usip_posegraph_optimize_f64(const int32_t* n, const int32_t* ecount, const int32_t* edge_i, const int32_t* edge_j,
                                const double* X, const double* info, const double* T0, int S, int Nmax, int Emax, double tau2,
                                double prune, int iterations1, int iterations2, void* workspace, long long workspace_bytes,
                                double* T, double* weight1, double* weight2, double* energy, uint8_t* kept,
                                int32_t* iterations_done, double* last_step, int32_t* status, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order, as plain loops; num_threads splits the
 * pairs or the scenes. */
int usip_icp_information_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                                 const int32_t* frag1, const int32_t* frag2, const int32_t* idx, const double* d2,
                                 const uint8_t* mask, int P, int Lmax, double radius, double* info, int32_t* count,
                                 int num_threads);
int usip_posegraph_optimize_f64_cpu(const int32_t* n, const int32_t* ecount, const int32_t* edge_i, const int32_t* edge_j,
                                    const double* X, const double* info, const double* T0, int S, int Nmax, int Emax,
                                    double tau2, double prune, int iterations1, int iterations2, double* T, double* weight1,
                                    double* weight2, double* energy, uint8_t* kept, int32_t* iterations_done,
                                    double* last_step, int32_t* status, int num_threads);

/* ------------------------------------------------------------------ f-16  baseline keypoints: Harris3D
 * The second hand-crafted detector the reference compares its learned one with (evaluation/save_keypoints.py:52-55, 303-313,
 * method = 'harris': PCLKeypoint.keypointHarris(xyz, radius 1, nms_threshold 0.001, threads 0)).  The PCL binding is not part
 * of the reference; the definition below is this project's own, written from PCL's HarrisKeypoint3D with method HARRIS, the
 * normals from NormalEstimation at the search radius, refineCorners off.  Float64 arithmetic on float32 inputs, never
 * contracted; every sum in ascending position of the frame's stable order along x; csrc/harris_math.h is the arithmetic.
 * Frames, count, perm, membership (strict d2 < r * r, the point itself a member) and the limits are f-11's.
 *
 * usip_harris_normals_f32: neighbours i32 [B][N] = m = |N_r(i)|; normals f64 [B][3][N]: zeros (NO NORMAL) when m <
 * min_neighbors; else, with d = p_j - p_i over N_r(i), s_a = sum d_a, s_ab = sum d_a d_b, c_ab = s_ab - (s_a * s_b) / m, the
 * eigenvector of the smallest eigenvalue of c / m by f-7's 8 cyclic Jacobi sweeps (the first of equal ones; (0, 0, 1) for a
 * zero trace), flipped towards the origin by f-7's rule (the first of the largest |components| c: negated when n[c] * p[c] >
 * 0).  A normal with a non-finite component is replaced by zeros.
 *
 * usip_harris_response_f32: normals f64 [B][3][N] as above or supplied (float32 normals cast to float64, used as given, not
 * renormalised).  A row HAS A NORMAL iff its three components are finite and not all zero.  A point without one: response 0,
 * members 0.  Else members i32 [B][N] = k = the members of N_r(i) that have a normal (>= 1) and, with C = (sum over them of
 * n_j n_j') / k, trace = (c00 + c11) + c22, det = ((((c00 c11) c22 + ((2 c01) c02) c12) - (c02 c02) c11) - (c01 c01) c22) -
 * (c12 c12) c00, response f64 [B][N] by method:
 *   0 HARRIS  (0.04 + det) - (0.04 * trace) * trace   (unit normals have trace 1, so this is det)
 *   1 NOBLE   det / trace
 *   2 LOWE    det / (trace * trace)
 *   3 TOMASI  the smallest eigenvalue of C (8 Jacobi sweeps)
 * a zero trace gives 0, a non-finite result gives 0.  tiles_visited as f-11's.
 *
 * Keypoints: i is one iff response[i] > 0, response[i] >= threshold (>= 0, the reference: 0.001) and no member of N_r(i) has a
 * larger response (equal ones do not suppress each other) -- usip_iss_nms_f32 with min_neighbors 1 on the response with
 * everything below the threshold set to 0.  Keypoints are cloud points: no refinement.
 * Slots beyond count[b] get zeros.  USIP_EINVAL: a shape outside the limits, min_neighbors < 1, an unknown method, a radius
 * that is not positive and finite, a NULL among the required pointers. */
int usip_harris_normals_f32(const float* pc, const int32_t* count, const int32_t* perm, int B, int N, double radius,
                            int min_neighbors, double* normals, int32_t* neighbours, void* stream);
int usip_harris_response_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* normals, int B, int N,
                             double radius, int method, double* response, int32_t* members, int32_t* tiles_visited,
                             void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order; every query tests all live points of its
 * frame, in the frame's own stable order along x (no perm); num_threads splits the queries. */
int usip_harris_normals_f32_cpu(const float* pc, const int32_t* count, int B, int N, double radius, int min_neighbors,
                                double* normals, int32_t* neighbours, int num_threads);
int usip_harris_response_f32_cpu(const float* pc, const int32_t* count, const double* normals, int B, int N, double radius,
                                 int method, double* response, int32_t* members, int num_threads);

/* ------------------------------------------------------------------ f-19  baseline descriptor: FPFH
 * The hand-crafted descriptor the reference's scoring scripts name beside the learned one (eval_indoor/3dmatch/evaluate.m,
 * evaluate_optimization.m, eval_loop.m: descriptorName = 'my'; % 3dmatch, spin, fpfh) and do not contain: Fast Point Feature
 * Histograms (Rusu, Blodow, Beetz 2009).  PCL is not part of the reference; the definition below is this project's own, written
 * after PCL's FPFHEstimation / computePairFeatures (DESIGN 8o lists the deviations).  Float64 arithmetic on float32 inputs,
 * never contracted; sqrt and division are the only operations beyond + - * and comparisons (no libm call feeds a decision or a
 * result); csrc/fpfh_math.h is the arithmetic.  Frames, count, perm, membership (strict d2 < r * r) and the limits are f-11's.
 *
 * Normals f64 [B][3][N] are f-16's (usip_harris_normals_f32, or float32 normals cast to float64 and used as given).  A row HAS A
 * NORMAL iff its components are finite and not all zero; a point without one is a member of nobody, its SPFH row is zero and
 * its member count 0.
 *
 * usip_fpfh_spfh_f32: members i32 [B][N] = the points j != i with a normal and d2(i, j) < r2 (a query counts every such row and
 * takes one off for itself); spfh i32 [B][N][33] = the INTEGER COUNTS of three 11-bin histograms over those members, bins h1 |
 * 11 + h2 | 22 + h3 of the pair (i, j).  With d = p_j - p_i, f4 = sqrt(d2): f4 == 0 adds to no bin.  a1 = (n_i . d) / f4, a2 =
 * (n_j . d) / f4 (dots as (a0 b0 + a1 b1) + a2 b2); |a1| < |a2|: n1 = n_j, n2 = n_i, d = -d, f3 = -a2; otherwise n1 = n_i, n2 =
 * n_j, f3 = a1.  v = d x n1; |v| == 0 adds to no bin; else v /= |v|, w = n1 x v, f2 = v . n2, y = w . n2, x = n1 . n2.  h2, h3 =
 * (11 (f + 1)) / 2 truncated and clamped to 0 .. 10.  h1 = the sector of width 2 pi / 11, counted from -pi, that holds the
 * direction (x, y), decided by the signs of cross products against ten boundary directions kept as float64 literals (no
 * inverse tangent); (0, 0) is bin 5, (x < 0, y == 0) is bin 10.  Integer counts do not depend on the order of the walk.
 * tiles_visited as f-11's.
 *
 * usip_fpfh_gather_f32: keypoints f32 [B][3][M] (any positions), kp_count i32 [B] or NULL.  Over the cloud points j with
 * members_j > 0 and 0 < d2(q, j) < r2 (kp_members i32 [B][M] counts them): sum[bin] += ((double)spfh_j[bin] * (100.0 /
 * members_j)) * (1.0 / d2).  THE ORDER OF THE SUMS: 64 partial sums; partial sum l takes the positions lo + l + 64 k of the
 * frame's stable order along x, ascending, lo = the first position with q_x - x < r; the 64 are folded by l += l ^ 32, 16, 8,
 * 4, 2, 1.  Each block of eleven is then multiplied by 100 / (its sum, bins ascending) when that sum is positive and zero
 * otherwise.  fpfh f64 [B][M][33].
 * Slots beyond count[b] / kp_count[b] get zeros.  USIP_EINVAL: a shape outside the limits (M in 1 .. 65535), a radius that is
 * not positive and finite, a NULL among the required pointers (count, kp_count and tiles_visited may be NULL). */
int usip_fpfh_spfh_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* normals, int B, int N,
                       double radius, int32_t* spfh, int32_t* members, int32_t* tiles_visited, void* stream);
int usip_fpfh_gather_f32(const float* pc, const int32_t* count, const int32_t* perm, const int32_t* spfh,
                         const int32_t* members, const float* keypoints, const int32_t* kp_count, int B, int N, int M,
                         double radius, double* fpfh, int32_t* kp_members, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order; every query and keypoint tests all live
 * points of its frame, in the frame's own stable order along x (no perm); num_threads splits the queries / keypoints. */
int usip_fpfh_spfh_f32_cpu(const float* pc, const int32_t* count, const double* normals, int B, int N, double radius,
                           int32_t* spfh, int32_t* members, int num_threads);
int usip_fpfh_gather_f32_cpu(const float* pc, const int32_t* count, const int32_t* spfh, const int32_t* members,
                             const float* keypoints, const int32_t* kp_count, int B, int N, int M, double radius, double* fpfh,
                             int32_t* kp_members, int num_threads);

/* ------------------------------------------------------------------ f-20  baseline descriptor: SHOT
 * The hand-crafted descriptor the reference's outdoor scoring script is set to (eval_outdoor/kitti/evaluate_kitti.m reads
 * .../kitti/shot/iss_256 with FEATURE_DIM = 352) and the reference does not contain: SHOT-352 (Tombari, Salti, Di Stefano 2010)
 * at keypoints of any detector.  PCL is not part of the reference; the definition below is this project's own, written after
 * PCL's SHOTEstimation / SHOTLocalReferenceFrameEstimation (DESIGN 8p lists the deviations).  Float64 arithmetic on float32
 * inputs, never contracted; only + - * / sqrt fabs and comparisons feed a result; csrc/shot_math.h is the arithmetic.  Frames,
 * count, perm, membership (strict d2 < r * r over f-7's sqdist(q, p_j)), the limits and the normals f64 [B][3][N] (a row HAS A
 * NORMAL iff its components are finite and not all zero) are f-19's; keypoints f32 [B][3][M] (any positions), kp_count i32 [B]
 * or NULL.  Every dot product is (a0 b0 + a1 b1) + a2 b2.
 *
 * usip_shot_lrf_f32: the local reference frame of keypoint q over ALL live rows within r (lrf_members i32 [B][M] counts them; no
 * normal is needed, a row at d2 == 0 counts).  d = p_j - q, w = r - sqrt(d2); seven sums: w, and with wda = w * da: wd0 d0,
 * wd0 d1, wd0 d2, wd1 d1, wd1 d2, wd2 d2.  THE ORDER OF THE SUMS is f-19's: 64 partial sums, partial sum l over the positions
 * lo + l + 64 k of the frame's stable order along x, ascending, lo = the first position with q_x - x < r; the 64 are folded by
 * l += l ^ 32, 16, 8, 4, 2, 1.  C = the six sums / sum w; f-7's 8 cyclic Jacobi sweeps in f-7's order; x = the eigenvector
 * column of the largest diagonal entry, z = of the smallest (the first of equal entries either way).  Sign of x: the members
 * with d . x >= 0 are counted against those with d . x < 0; x is negated iff the first count is the smaller (a tie keeps x); z
 * likewise; y = z cross x.  lrf f64 [B][M][9] = the rows x, y, z.  Fewer than 5 members, a sum w that is not positive or a
 * component that is not finite: NO FRAME, nine zeros.
 *
 * usip_shot_hist_f32: lrf f64 [B][M][9] as above or supplied; a row of it IS A FRAME iff its nine numbers are finite and x is
 * not all zero.  The members of q: rows with a normal, d2 < r2 and d2 > 0 (kp_members i32 [B][M] counts them, with or without
 * a frame).  x' = d . x, y' = d . y, z' = d . z, dist = sqrt(d2), c = n_j . z clamped to [-1, 1].
 *   hard bins   t = (1 + c) * 5, cb = (int)(t + 0.5) in 0 .. 10; sh = dist > r / 2; el = z' > 0; az = the sector of width pi / 4,
 *               counted from -pi, that holds the direction (x', y'), decided by signs and |x'| against |y'| alone.  THE TIE RULE:
 *               a boundary direction belongs to the sector that begins there, the direction pi (y' == 0 of either sign, x' < 0)
 *               to sector 7, (0, 0) is the direction 0 (sector 4): with y' >= 0, x' > 0 gives 4 when |y'| < |x'| and 5
 *               otherwise, x' <= 0 gives 6 when |y'| > |x'| and 7 otherwise; with y' < 0, x' < 0 gives 0 when |y'| < |x'| and 1
 *               otherwise, x' >= 0 gives 2 when |y'| > |x'| and 3 otherwise.  column = ((az * 2 + el) * 2 + sh) * 11 + cb.
 *   offsets     from the centre of the member's own bin, each clamped to [-1/2, 1/2].  cosine: t - cb, neighbour cb + 1 or cb -
 *               1 by its sign where that lies in 0 .. 10.  radial: dist / (r / 2) - 1/2 (inner shell; neighbour the outer shell
 *               for an offset > 0) or (dist - r / 2) / (r / 2) - 1/2 (outer shell; neighbour the inner shell for an offset < 0);
 *               no neighbour towards the centre or beyond r.  elevation: u = z' / dist clamped to [-1, 1], theta =
 *               angle(sqrt((1 - u) * (1 + u)), u), offset (theta - centre) / (pi / 2) with centre pi / 4 (el = 1) or 3 pi / 4
 *               (el = 0); the neighbour is the other half on the equator side only (el = 1: offset > 0; el = 0: offset < 0).
 *               azimuth: phi = angle(y', x'), offset (phi - (az - 3.5) * (pi / 4)) / (pi / 4), neighbour az + 1 or az - 1 modulo 8
 *               by its sign.  angle(y, x) is csrc/shot_math.h's own inverse tangent of two arguments (an octant reduction by
 *               comparisons, one division, a float64 polynomial in Horner's order), the same operations on either side; a zero
 *               of either sign counts as +0.
 *   weights     INTEGERS, quantum 2^-32: q_k = (int64)(|offset_k| * 4294967296.0); the member's own column gets the sum over
 *               the four k of 2^32 - q_k, each existing neighbour column its q_k; a q_k towards a missing neighbour is dropped.
 *               hist i64 [B][M][352].  Integer sums do not depend on the order of the walk.
 *   descriptor  h_b = (double)hist_b; s = sum h_b * h_b: 64 partial sums, partial l over the columns l + 64 k ascending,
 *               folded as above; shot f64 [B][M][352] = h / sqrt(s), zeros when s == 0 or there is no frame.
 * Slots beyond kp_count[b] get zeros.  A wrong perm gives wrong values, never a wild read.  USIP_EINVAL: a shape outside the
 * limits (M in 1 .. 65535), a radius that is not positive and finite, a NULL among the required pointers (count and kp_count
 * may be NULL). */
int usip_shot_lrf_f32(const float* pc, const int32_t* count, const int32_t* perm, const float* keypoints,
                      const int32_t* kp_count, int B, int N, int M, double radius, double* lrf, int32_t* lrf_members,
                      void* stream);
int usip_shot_hist_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* normals,
                       const float* keypoints, const int32_t* kp_count, const double* lrf, int B, int N, int M, double radius,
                       int64_t* hist, double* shot, int32_t* kp_members, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order; every keypoint tests all live points of its
 * frame, in the frame's own stable order along x (no perm); num_threads splits the keypoints. */
int usip_shot_lrf_f32_cpu(const float* pc, const int32_t* count, const float* keypoints, const int32_t* kp_count, int B, int N,
                          int M, double radius, double* lrf, int32_t* lrf_members, int num_threads);
int usip_shot_hist_f32_cpu(const float* pc, const int32_t* count, const double* normals, const float* keypoints,
                           const int32_t* kp_count, const double* lrf, int B, int N, int M, double radius, int64_t* hist,
                           double* shot, int32_t* kp_members, int num_threads);
/* out[i] = angle(y[i], x[i]), i < n: the inverse tangent as either side evaluates it, for measuring it against a libm */
int usip_shot_angle_f64_cpu(const double* y, const double* x, long long n, double* out);

/* ------------------------------------------------------------------ f-21  baseline descriptor: spin images
 * The last hand-crafted descriptor the reference's indoor scoring scripts name (eval_indoor/3dmatch/evaluate.m,
 * evaluate_optimization.m, loop_evaluation/eval_loop.m: descriptorName = 'my'; % 3dmatch, spin, fpfh) and the reference does not
 * contain: spin images (Johnson, Hebert 1999) at keypoints of any detector.  PCL is not part of the reference; the definition
 * below is this project's own, written after PCL's SpinImageEstimation (DESIGN 8q lists the deviations).  Float64 arithmetic on
 * float32 inputs, never contracted; only + - * / sqrt fabs floor and comparisons feed a result; csrc/spin_math.h is the
 * arithmetic.  Frames, count, perm, membership (strict d2 < r * r over f-7's sqdist(q, p_j)), the limits, keypoints f32
 * [B][3][M] (any positions) and kp_count are f-20's.  Every dot product is (a0 b0 + a1 b1) + a2 b2.
 *
 * usip_spin_image_f32:
 *   axis        a row v of axes f64 [B][M][3] (f-20's z row, lrf[..][6 .. 8], or the caller's) IS AN AXIS iff its three numbers
 *               are finite and v . v is positive and finite; a = v / sqrt(v . v).  Without an axis: zeros, no member.
 *   members     live rows with d2 > 0 and d2 < r * r.  d = p_j - q, beta = d . a.  With support_angle_cos = s > 0: normals f64
 *               [B][3][N] as f-19's; a row without a normal is skipped and so is one with fabs(n_j . a) < s (a counter-directed
 *               normal passes); normals are used as given.  With s == 0 no normal is read and normals may be NULL.
 *   structure 0 (rectangular) W = 8, bin = (r * 0.70710678118654757) / W: the cylinder inscribed in the search sphere.  alpha =
 *               sqrt(max(0, d2 - beta * beta)), u = alpha / bin, v = beta / bin; the row is a member iff u < W, v < W and v > -W.
 *   structure 1 (radial) bin = r / W, u = sqrt(d2) / bin; c = beta / sqrt(d2) clamped to [-1, 1], theta = angle(c, sqrt((1 - c) *
 *               (1 + c))), f-20's inverse tangent: the arc sine of c in [-pi / 2, pi / 2]; v = theta / ((pi / 2) / W).  Every row
 *               of the sphere is a member; a u that reaches W after rounding goes to ab = W - 1 and a v that reaches W to bb =
 *               2 W - 1, with the largest offset below 1 (2^20 - 1 quanta).
 *   cells       ab = (int)floor(u), bb = (int)floor(v) + W, offsets u - floor(u) and v - floor(v).
 *   weights     INTEGERS, quantum 2^-20 per axis: qa = (int64)(offset_a * 1048576.0) capped at 2^20 - 1, qb likewise; the cells
 *               (ab, bb), (ab + 1, bb), (ab, bb + 1), (ab + 1, bb + 1) get (2^20 - qa)(2^20 - qb), qa (2^20 - qb), (2^20 - qa) qb,
 *               qa qb: exactly 2^40 per member.  column = row * (2 W + 1) + col: hist i64 [B][M][153] (9 rows of alpha, 17
 *               columns of beta).  N <= 2^20 keeps a row's total below 2^61.  Integer sums do not depend on the order of the walk.
 *   descriptor  kp_members i32 [B][M] counts the rows that added; spin f64 [B][M][153] = (double)hist_b / ((double)kp_members *
 *               2^40), zeros when kp_members == 0.
 * Slots beyond kp_count[b] get zeros.  A wrong perm gives wrong values, never a wild read.  USIP_EINVAL: a shape outside the
 * limits (M in 1 .. 65535), a radius that is not positive and finite, support_angle_cos outside [0, 1] or not finite,
 * support_angle_cos > 0 with normals NULL, a structure other than 0 and 1, a NULL among the required pointers (count, kp_count
 * and, without a support angle, normals may be NULL). */
int usip_spin_image_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* normals,
                        const float* keypoints, const int32_t* kp_count, const double* axes, int B, int N, int M, double radius,
                        double support_angle_cos, int structure, int64_t* hist, double* spin, int32_t* kp_members, void* stream);
/* HOST twin (every pointer on the host): the same arithmetic; every keypoint tests all live points of its frame, in the
 * frame's own stable order along x (no perm); num_threads splits the keypoints. */
int usip_spin_image_f32_cpu(const float* pc, const int32_t* count, const double* normals, const float* keypoints,
                            const int32_t* kp_count, const double* axes, int B, int N, int M, double radius,
                            double support_angle_cos, int structure, int64_t* hist, double* spin, int32_t* kp_members,
                            int num_threads);

/* ------------------------------------------------------------------ f-17  baseline keypoints: SIFT3D
 * The third hand-crafted detector the reference compares its learned one with (evaluation/save_keypoints.py:57-61, 314-325,
 * method = 'sift': PCLKeypoint.keypointSift(xyz, min_scale 0.5, n_octaves 4, n_scales_per_octave 8, min_contrast 0.1)).  The
 * PCL binding is not part of the reference and receives nothing but xyz, so the field of the scale space can only be a
 * function of a coordinate; here it is an axis of the cloud (z by default, PCL's selector for xyz-only clouds) or a float32
 * scalar per point.  The definition below is this project's own, written from PCL's SIFTKeypoint.  Float64 arithmetic on
 * float32 inputs, never contracted; every sum in the stated order; csrc/sift_math.h is the arithmetic.  Frames (pc f32
 * [B][3][N], count i32 [B] or NULL) and the limits (N <= 2^20, B <= 65535) are f-11's.
 *
 * Octaves.  base_o = min_scale * 2^o, o < n_octaves <= 8.  Octave 0's cloud is the voxel average of the input at leaf base_0,
 * octave o's the voxel average of octave o-1's cloud at leaf base_o (keypoints are cell centroids, not cloud points).
 * usip_sift_voxel_keys_f32: keys i64 [B][N]; cell = floor(v / leaf) per axis in float64 (grid anchored at the origin); key =
 * (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20); a cell index outside [-2^20, 2^20), a non-finite coordinate or a slot
 * beyond count[b] gives INT64_MAX, which drops the row.
 * usip_sift_voxel_average_f32: sorted_keys i64 [B][N] = every frame's keys ascending and order i32 [B][N] = the input index of
 * each (a STABLE sort: equal keys in ascending input index).  Row c of the output is the c-th distinct key: out_pc f32
 * [B][3][N] = the float64 sum of its members in that order / their count, cast to float32; out_field f32 [B][N] = that row's
 * own float32 coordinate `axis` (0, 1, 2) when field is NULL, else the members' float64 mean of field f32 [B][N] cast to
 * float32; count_out i32 [B] = the distinct keys; rows beyond it are zeros.  No host read.
 *
 * Scales.  S = n_scales_per_octave + 3 in 4 .. 11; sigma_s = base_o * 2^((s - 1) / n_scales_per_octave).  sigma2 f64 [S] ON THE
 * HOST holds sigma_s^2, computed once by the caller and handed to the kernel and the twin alike (positive, finite, ascending).
 *
 * A cloud with fewer than 25 points is EMPTY for the three entry points below: everything zero.  Counts only shrink from
 * octave to octave, so this is PCL's `break` without a host read.
 * usip_sift_dog_f32: perm i32 [B][N] = the frame's live rows ascending along x (stable), as f-11's.  The members of (i, s):
 * d2(i, j) < 9 * sigma_s^2 with d2 f-7's sqdist (strict; the point itself is one); w = sift_exp(-((0.5 * d2) / sigma_s^2));
 * num_s += f_j * w, den_s += w in ascending position of perm; G_s = num_s / den_s; dog f64 [B][S-1][N] = G_{s+1} - G_s at the
 * cloud's own rows.  sift_exp is csrc/sift_math.h's float64 exponential (range reduction by ln 2, degree-13 Taylor in Horner's
 * order, ldexp), the same operations on either side.  The walk's radius is the smallest r >= sqrt(9 sigma_{S-1}^2) with r * r
 * >= 9 sigma_{S-1}^2; tiles_visited i32 [B][ceil(N/256)] or NULL as f-11's.
 * usip_sift_nearest_f32: idx i32 [B][N][25] = the 25 nearest rows of row i, itself included, ascending (d2, row).
 * usip_sift_extrema_f32: for s = 1 .. S-3 and v = dog[s][i]: extremal iff |v| >= min_contrast and (v == min_s and v < min_{s-1}
 * and v < min_{s+1}) or (v == max_s and v > max_{s-1} and v > max_{s+1}), minima and maxima over the 25 rows of idx.  mask u8
 * [B][N] = extremal at some s; scale_index i32 [B][N] = the lowest such s, 0 when there is none.
 * USIP_EINVAL: a shape outside the limits, S outside 4 .. 11, a leaf or a sigma2 that is not positive and finite, sigma2 not
 * ascending, axis outside 0 .. 2, min_contrast not >= 0, a NULL among the required pointers. */
int usip_sift_voxel_keys_f32(const float* pc, const int32_t* count, int B, int N, double leaf, int64_t* keys, void* stream);
int usip_sift_voxel_average_f32(const float* pc, const float* field, int axis, const int64_t* sorted_keys, const int32_t* order,
                                int B, int N, float* out_pc, float* out_field, int32_t* count_out, void* stream);
int usip_sift_dog_f32(const float* pc, const float* field, const int32_t* count, const int32_t* perm, int B, int N, int S,
                      const double* sigma2, double* dog, int32_t* tiles_visited, void* stream);
int usip_sift_nearest_f32(const float* pc, const int32_t* count, const int32_t* perm, int B, int N, int32_t* idx, void* stream);
int usip_sift_extrema_f32(const double* dog, const int32_t* idx, const int32_t* count, int B, int N, int S, double min_contrast,
                          uint8_t* mask, int32_t* scale_index, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order.  The voxel average takes the UNSORTED keys and
 * sorts them itself; the scale space and the 25 nearest offer all live rows of the frame to every query in the frame's own
 * stable order along x (no perm); num_threads splits the queries (the cells). */
int usip_sift_voxel_keys_f32_cpu(const float* pc, const int32_t* count, int B, int N, double leaf, int64_t* keys);
int usip_sift_voxel_average_f32_cpu(const float* pc, const float* field, int axis, const int64_t* keys, int B, int N,
                                    float* out_pc, float* out_field, int32_t* count_out, int num_threads);
int usip_sift_dog_f32_cpu(const float* pc, const float* field, const int32_t* count, int B, int N, int S, const double* sigma2,
                          double* dog, int num_threads);
/* out[i] = sift_exp(x[i]), i < n: the exponential as either side evaluates it, for measuring it against a libm */
int usip_sift_exp_f64_cpu(const double* x, long long n, double* out);
int usip_sift_nearest_f32_cpu(const float* pc, const int32_t* count, int B, int N, int32_t* idx, int num_threads);
int usip_sift_extrema_f32_cpu(const double* dog, const int32_t* idx, const int32_t* count, int B, int N, int S,
                              double min_contrast, uint8_t* mask, int32_t* scale_index, int num_threads);

/* ------------------------------------------------------------------ f-18  a fragment scene's ground truth: gt.log and gt.info
 * The files every indoor number is scored against come from evaluation/matlab/eval_indoor/3dmatch/getGtInfoLog.m: for every
 * pair i < j of a scene's fragments, relExt = inv(T_i) T_j from the fragments' camera-to-world poses, fragment j moved by it,
 * for every moved row the distance d to the nearest row of fragment i (both clouds grid-averaged at 0.01 m), alignedRatio =
 * #{d < 0.03} / (rows of fragment i) (the count is over fragment j's rows, the denominator fragment i's length: the reference's
 * rule), the pair kept at alignedRatio >= 0.3, covMat = the sum of G'G, G = [I3 | -[q]x], over the moved rows q with d <
 * 0.006, thinned to 5000 rows when there are more.  f-9's conventions: float64 arithmetic on float32 rows, never contracted,
 * the moved point by f-9's xform, the strict sqrt(d2) < radius of f-9's within, every sum in a stated order, no floating-point
 * atomics, no launch synchronises the host, every index read from memory is clamped.  csrc/ground_truth_math.h is the
 * arithmetic.  MATLAB's pcdownsample 'random' draws from a stream that cannot be reproduced; the thinning here is this
 * project's own: a key per near row, the `cap` smallest (key, row) kept.
 *
 * The bank and the pairs are f-13's: rows, row_len, offsets, num_frags, total_rows, perm1 i32 [total_rows]; frag1, frag2 i32
 * [P] (clamped into the bank), Rt f64 [P][3][4] moving fragment 2 (n2 rows) into fragment 1's frame (n1 rows), mask u8 [P]
 * (NULL: all ones), Lmax at least the length of every fragment a pair names.
 *
 * usip_gt_reach_f32: perm2 i32 [P][Lmax]: fragment 2's local row indices ascending along the moved x (usip_overlap_keys_f32 and
 * a stable sort); it decides which rows share a workgroup and, as long as its first n2 slots hold a permutation, never a
 * result (values are clamped; a row no slot names keeps cls 0 and the key of a row that is not near).  With q = R b_i + t and
 * d2_i the least sqdist3(q, a_j) over the rows of fragment 1:
 *   cls u8 [P][Lmax], in fragment 2's LOCAL row order: 2 when sqrt(d2_i) < near_radius, else 1 when sqrt(d2_i) < far_radius,
 *     else 0; zeros beyond n2.  The answer is the all-pairs one as long as perm1 sorts: a tile of fragment 1 is skipped only
 *     when its x-gap alone reaches far_radius (f-9's beyond), a row is no longer tested only once its class is 2.
 *   hits i32 [P][2] = #{cls >= 1}, #{cls == 2}; ratio f64 [P][2] = hits[p][0] / n1 (the reference's alignedRatio), hits[p][0] /
 *     n2; 0 for an empty fragment.
 *   key u64 [P][Lmax]: for a row with cls 2 the first word of the Philox4x64-10 block (csrc/pairs_rng.h) of counter (i, 0,
 *     pair id, 0) under key (seed, 0x67745f6b6579), shifted right by one bit; all ones for every other row and beyond n2 --
 *     sorted ascending (stable) the near rows come first, the lower row among equal keys, and no near row's key equals the
 *     padding's.  pair_ids i64 [P] (NULL: p): a pair's keys depend on (seed, pair id, row) only, never on P or the batch.
 * A pair with mask 0, n1 = 0 or n2 = 0 gets cls 0, key all ones, hits 0, ratio 0.
 *
 * usip_gt_information_f32: order i32 [P][cap]: local rows of fragment 2 (clamped into it), count i32 [P] (clamped into 0 ..
 * cap) -> info f64 [P][6][6] = the sum over s < count of G'G at q = R b_order[s] + t: the count, the three sums of q and the
 * six distinct entries of [q]x'[q]x (qz qz + qy qy, qz qz + qx qx, qy qy + qx qx, qx qy, qx qz, qy qz); lane l of 256 adds
 * positions l, l + 256, ... in ascending s, the 256 partial sums go through f-6's binary tree, the matrix is assigned entry
 * by entry and so exactly symmetric.  G has no factor 2: this is not usip_information_f32's A.  A pair with count 0 (what a
 * masked, empty or hit-less pair has after usip_gt_reach_f32) or n2 = 0 gets zeros, never a NaN.
 *
 * USIP_EINVAL: the bank's and P's limits of f-13, radii that are not positive or far_radius <= near_radius, cap outside 1 ..
 * 65536, a NULL among the required pointers. */
int usip_gt_reach_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                      const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt, const int32_t* perm2,
                      const uint8_t* mask, int P, int Lmax, double far_radius, double near_radius, uint64_t seed,
                      const int64_t* pair_ids, uint8_t* cls, int32_t* hits, double* ratio, uint64_t* key, void* stream);
int usip_gt_information_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                            const int32_t* frag2, const double* Rt, const int32_t* order, const int32_t* count, int P, int Lmax,
                            int cap, double* info, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order.  The reach twin takes no perm2: it tests the
 * rows of fragment 1 for every row of fragment 2 in ascending row order -- all of them with prune = 0, otherwise outward along
 * x (perm1) until the gap alone reaches far_radius.  num_threads splits the pairs. */
int usip_gt_reach_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                          const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt, const uint8_t* mask,
                          int P, int Lmax, double far_radius, double near_radius, uint64_t seed, const int64_t* pair_ids,
                          int prune, uint8_t* cls, int32_t* hits, double* ratio, uint64_t* key, int num_threads);
int usip_gt_information_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                                const int32_t* frag2, const double* Rt, const int32_t* order, const int32_t* count, int P,
                                int Lmax, int cap, double* info, int num_threads);

/* ------------------------------------------------------------------ f-22  the indoor descriptor's loss: CGF triplets
 * losses.DescCGFLoss (models/losses.py:240-314) without its B x C x M x M difference tensor, its B x M x M norm and its three
 * random B x M x M matrices: the three indices it reads per anchor depend on the keypoints and the random numbers only, the
 * loss needs three C-long distances per anchor, and the backward pass scatters three unit vectors.  csrc/cgf_math.h is the
 * arithmetic.  anc_kp, pos_kp f32 [B][3][M] (anc_kp already in the positive's frame), anc_desc, pos_desc f32 [B][C][M],
 * anc_sigma f32 [B][M].  1 <= B, 1 <= M <= 65535, 1 <= C <= 4096, radius > 0 (also as a float32).
 *
 * usip_cgf_select_f32: float32 decisions, as the reference's.  For anchor i and candidate j: d_ij = sqrtf((dx dx + dy dy) + dz
 * dz), never contracted; pos_ij = d_ij <= (float)radius; has_i = any_j pos_ij; j_pos = argmax_j (pos_ij ? u1_ij : 0); j_far =
 * argmin_j of the float32 value d_ij + (pos_ij ? 1000.f : 0.f) -- the one float32 add, with its quantisation, is the
 * reference's and decides the all-inside row as it does; j_out = argmax_j (d_ij > (float)radius ? u2_ij : 0); every tie goes
 * to the LOWEST j, so an all-zero row gives 0; a NaN key is never chosen and a row of NaN keys gives 0.  take_far_i = u3_i <
 * 0.5f; j_neg = take_far ? j_far : j_out.  sel i32 [B][M][3] = (j_pos, j_far, j_out); has, take_far u8 [B][M].
 * Draws: u1, u2 f32 [B][M][M] and u3 f32 [B][M], all three or none (the recorded draws of the reference: tests only).  None:
 * Philox4x64-10 (csrc/pairs_rng.h), key (seed, "cgf_loss"), counter (i << 16 | j, 27 << 8, elem_base + b, step) -> words 0, 1
 * give u1_ij, u2_ij; counter (i, 27 << 8 | 1, elem_base + b, step) -> word 0 gives u3_i; a uniform is the word's top 24 bits
 * times 2^-24 (exact in float32, in [0, 1)).  A draw depends on (seed, step, elem_base + b, i, j) only: never on B, the rank
 * split or the launch.  step_dev, when not NULL, is a DEVICE word read by the kernel in place of `step`: a captured graph
 * draws fresh numbers on every replay after the caller increments the word.
 *
 * usip_cgf_loss_f32: float64 arithmetic from the float32 inputs, never contracted, f-9's conventions; indices read from sel
 * are clamped into 0 .. M-1.  D(i, j) = sqrt(sum_c (a_ci - p_cj)^2): lane l of 64 adds channels l, l + 64, ... ascending, the 64
 * partial sums go through the binary tree part[l] += part[l + s], s = 32 .. 1.  dist f64 [B][M][2] = D(i, j_pos), D(i, j_neg),
 * for every anchor.  n_b = sum_i has_i; before_i = has_i ? (D(i, j_pos) - D(i, j_neg)) + gamma : 0; active f32 [B] = #{before_i >
 * 1e-5} / (n_b + 1); raw_i = max(sigma_max - sigma_i, 0); mean_b = (sum_i raw_i) / M, the sum as 256 strided partial sums in
 * ascending i and the same kind of tree; w_i = raw_i / mean_b, and 0 when mean_b is 0 (every sigma at or above sigma_max: the
 * reference divides 0 by 0 and returns NaN; here the row is 0); coef f64 [B][M] = (w_i * M) / (n_b + 1) where before_i > 0, else
 * 0; loss f32 [B][M] = coef_i * before_i where before_i > 0, else 0; loss and active are rounded once.
 *
 * usip_cgf_loss_backward_f32: grad_loss f32 [B][M]; g_i = grad_loss_i * coef_i; unit(v) = v / |v| with the saved distance, ZERO
 * at distance 0 (torch's norm backward).  d_anc[:, i] = g_i * (unit(a_i - p_jpos) - unit(a_i - p_jneg)).  d_pos[:, j] = the sum
 * over the anchors i ascending of -(g_i * unit(a_i - p_j)) when j_pos(i) == j, followed by +(g_i * unit(a_i - p_j)) when j_neg(i)
 * == j, from 0, rounded once; no floating-point atomics.  Keypoints and sigmas receive no gradient (the reference detaches
 * the weights; masks and arg-mins carry none).
 *
 * No launch synchronises the host; no B x M x M or B x C x M x M array exists on the Philox path.  USIP_EINVAL: a shape outside
 * the limits, a radius that is not positive, some but not all of u1, u2, u3, a NULL among the required pointers. */
int usip_cgf_select_f32(const float* anc_kp, const float* pos_kp, int B, int M, double radius, const float* u1, const float* u2,
                        const float* u3, uint64_t seed, uint64_t step, const uint64_t* step_dev, uint64_t elem_base, int32_t* sel,
                        uint8_t* has, uint8_t* take_far, void* stream);
int usip_cgf_loss_f32(const float* anc_desc, const float* pos_desc, const float* anc_sigma, const int32_t* sel, const uint8_t* has,
                      const uint8_t* take_far, int B, int M, int C, double gamma, double sigma_max, float* loss, float* active,
                      double* dist, double* coef, void* stream);
int usip_cgf_loss_backward_f32(const float* anc_desc, const float* pos_desc, const int32_t* sel, const uint8_t* take_far,
                               const double* dist, const double* coef, const float* grad_loss, int B, int M, int C, float* d_anc,
                               float* d_pos, void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same orders; num_threads splits the anchors (the columns
 * of d_pos).  The selection twin takes `step` by value only. */
int usip_cgf_select_f32_cpu(const float* anc_kp, const float* pos_kp, int B, int M, double radius, const float* u1, const float* u2,
                            const float* u3, uint64_t seed, uint64_t step, uint64_t elem_base, int32_t* sel, uint8_t* has,
                            uint8_t* take_far, int num_threads);
int usip_cgf_loss_f32_cpu(const float* anc_desc, const float* pos_desc, const float* anc_sigma, const int32_t* sel,
                          const uint8_t* has, const uint8_t* take_far, int B, int M, int C, double gamma, double sigma_max,
                          float* loss, float* active, double* dist, double* coef, int num_threads);
int usip_cgf_loss_backward_f32_cpu(const float* anc_desc, const float* pos_desc, const int32_t* sel, const uint8_t* take_far,
                                   const double* dist, const double* coef, const float* grad_loss, int B, int M, int C,
                                   float* d_anc, float* d_pos, int num_threads);

/* ------------------------------------------------------------------ f-25  the indoor head's last line: unit columns
 * out = x / (|x| + eps), the norm over the channels (models/networks.py:477), and its backward, one launch each.
 * csrc/unit_math.h is the arithmetic.  x, out, grad, dx f32 [B][C][M]; norm f32 [B][M]; every buffer contiguous.
 *
 * usip_unit_columns_f32: per position (b, m): s = sum_c (double)x_c * (double)x_c in ascending c from 0; n = (float)sqrt(s),
 * stored in norm; t = n + eps in float32; out_c = x_c / t in float32.
 * usip_unit_columns_backward_f32: norm is the forward's; dot = sum_c (double)grad_c * (double)x_c in ascending c; t = n + eps in
 * float32; in float64, dx_c = (float)(grad_c / t - (x_c * dot) / ((n * t) * t)), and (float)(grad_c / t) where n == 0 (torch's
 * zero sub-gradient of the norm).
 * NaN and Inf propagate with no special case, inside their own column.  One lane per position walks the channels, so no sum
 * depends on the launch geometry; one-dimensional grid, with a loop beyond 65536 workgroups of 64.
 * B * M == 0 returns USIP_OK and launches nothing (C == 0 with positions writes norm = 0).  USIP_EINVAL: a negative B, C or
 * M, an eps that is negative or NaN, a NULL pointer. */
int usip_unit_columns_f32(const float* x, int B, int C, int M, float eps, float* out, float* norm, void* stream);
int usip_unit_columns_backward_f32(const float* grad, const float* x, const float* norm, int B, int C, int M, float eps, float* dx,
                                   void* stream);
/* HOST twins (every pointer on the host): the same arithmetic in the same order; num_threads splits the positions. */
int usip_unit_columns_f32_cpu(const float* x, int B, int C, int M, float eps, float* out, float* norm, int num_threads);
int usip_unit_columns_backward_f32_cpu(const float* grad, const float* x, const float* norm, int B, int C, int M, float eps,
                                       float* dx, int num_threads);

/* ------------------------------------------------------------------ f-28  trimmed ICP under the point-to-plane metric
 * pcregrigid's 'Metric' option 'pointToPlane' for the refinement of f-13: every kept row of B is drawn towards the PLANE
 * through its nearest row of A instead of towards that row, so a cloud may slide along a wall while it is still off it.
 * pcregrigid is a MATLAB built-in; the definition is this project's own (the linearised point-to-plane fit of Chen and
 * Medioni 1992 as Low 2004 states it, one Gauss-Newton step per iteration).  f-13's conventions apply word for word: float32
 * inputs, float64 arithmetic, never contracted, sums in a fixed order, no floating-point atomics, no launch synchronises the
 * host, every index read from memory is clamped before use.  csrc/icp_plane_math.h is the arithmetic.
 *
 * The bank is f-13's with row_len >= 6: x y z, then the row's unit normal nx ny nz in float32 (f-7's scan normals of the
 * DOWNSAMPLED rows: fragments.RefineBank(normals=True)); row_len < 6 is USIP_EINVAL.  Only the normals of A are read.
 *
 * usip_icp_refine_plane_f32 is f-13's loop with another step 3.  Steps 1, 2 and 5, the final pass, mask, order2, Lmax,
 * cut_d2 / cut_i, visits, stage_ms, the workspace and the limits are f-13's: the trim stays on the POINT distance d2, rmse
 * stays the root mean kept d2.  Step 3 under the current pose (R, t), for every kept row i of B in f-13's lane-strided order
 * (lane l of 256 adds its kept rows among l, l + 256, ... in ascending i, then f-6's binary tree, each of the 27 columns alone):
 *    q = R b_i + t by f-9's xform (the bits the search used); a, n = the position and normal of row idx[i] of A, widened;
 *    c = (q1 n2 - q2 n1, q2 n0 - q0 n2, q0 n1 - q1 n0);  J = (c0, c1, c2, n0, n1, n2);
 *    r = ((q0 - a0) n0 + (q1 - a1) n1) + (q2 - a2) n2;
 *    27 sums: the 21 entries H_jk += J_j J_k (j <= k, row-major), then the six g_j += J_j r.
 * H x = -g is solved by a Cholesky factorisation written as f-12's solve6 is, for a full upper triangle: the factor column by
 * column, inner sums subtracted in ascending k, then the forward and the backward substitution.  The new pose is f-12's
 * apply_step: R <- D R, t <- D t + x3..5 with D = Rz(x2) Ry(x1) Rx(x0) from f-12's sine and cosine.
 * A solve FAILS on a pivot that is not finite and positive, a component of x that is not finite, or |x0..2| > pi.  A failed
 * solve ends the pair exactly as f-13's rule 4 does: the last pose stays, converged = 0, iterations = k - 1, and the final
 * pass still runs.  There is no damping and no fallback to the other metric: a fragment whose normals are all zero (fewer
 * rows than the normals need), all parallel (one wall) or all in one plane (two walls) fails its first solve and keeps Rt0.
 * Negating any of the normals changes no bit of any output: J and r change sign together, and every sum is of their products.
 *
 * fit_sums f64 [P][max_iterations][27], optional (NULL): the 27 sums of every fit that ran -- the one whose solve failed
 * included -- fit k at [k - 1], zeros elsewhere; what cut_d2 / cut_i are for the trim. */
int usip_icp_refine_plane_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                              const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt0,
                              const uint8_t* mask, const int32_t* order2, int P, int Lmax, double inlier_ratio,
                              int max_iterations, double tol_t, double tol_c, double align_radius, void* workspace,
                              long long workspace_bytes, double* Rt, int32_t* iterations, uint8_t* converged, double* rmse,
                              int32_t* hits, double* ratio, double* cut_d2, int32_t* cut_i, unsigned long long* visits,
                              double* stage_ms, double* fit_sums, void* stream);
/* HOST twin (every pointer on the host), as usip_icp_refine_f32_cpu is f-13's. */
int usip_icp_refine_plane_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                                  const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt0,
                                  const uint8_t* mask, const int32_t* order2, int P, int Lmax, double inlier_ratio,
                                  int max_iterations, double tol_t, double tol_c, double align_radius, double* Rt,
                                  int32_t* iterations, uint8_t* converged, double* rmse, int32_t* hits, double* ratio,
                                  double* cut_d2, int32_t* cut_i, int32_t* idx_out, double* d2_out, double* fit_sums,
                                  int num_threads);

#ifdef __cplusplus
}
#endif
#endif /* USIP_HIP_H */
