/*
 * s2d.h — C-ABI of libs2d_hip.so: the MI355X (gfx950) hot path of Sparse2Dense / CenterPoint.
 *
 * One `extern "C"` shared object, plain pointers and sizes only (no torch / C++ types).  It
 * replaces, for the voxel-backbone path, what the reference binds through numba and through the
 * third-party `spconv` extension (reference = /root/reference, stevewongv/Sparse2Dense):
 *
 *   s2d_voxelize_*        <- det3d/ops/point_cloud/point_cloud_ops.py:7-55,112-184
 *                            (points_to_voxel / _points_to_voxel_reverse_kernel) fused with
 *                            det3d/models/readers/voxel_encoder.py:17-24 (per-voxel mean)
 *   s2d_rulebook_subm_*   <- spconv.ops.get_indice_pairs(subm=True)  as called by SubMConv3d at
 *                            det3d/models/backbones/scn.py:18-26,105,202-238
 *   s2d_rulebook_conv_*   <- spconv.ops.get_indice_pairs(subm=False) as called by SparseConv3d at
 *                            det3d/models/backbones/scn.py:116-118,126-128,136-138,147-149
 *   s2d_spconv_fwd / _wgrad <- spconv.ops.indice_conv / indice_conv_backward (same call sites)
 *   s2d_bn1d_*            <- nn.BatchNorm1d + ReLU + residual on `.features`, scn.py:69-85,104-152
 *   s2d_densify_*         <- spconv.SparseConvTensor.dense(), scn.py:173-176, voxelnet.py:203-215
 *
 * Conventions
 *   - every entry returns int: 0 = OK, <0 = invalid argument / unsupported shape / capacity,
 *     >0 = hipError_t of a failed HIP call; text via s2d_last_error() (thread-local).
 *   - all buffers are caller-owned DEVICE pointers (PyTorch caching allocator in our host code);
 *     the library never allocates, frees or retains device memory.
 *   - every entry is asynchronous on the caller's stream (`s2d_stream_t` = hipStream_t passed as
 *     void*; NULL = the null stream) and never synchronises the device.
 *   - variable-size results use a device scalar (`out_m`, `out_n`) that the HOST reads back only
 *     where the reference API itself exposes a size.
 *   - indices are int32, features fp32 (bf16 entry points carry the _bf16 suffix).
 */
#ifndef S2D_H_
#define S2D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *s2d_stream_t;

#define S2D_OK 0
#define S2D_ERR_INVALID_ARG (-1)
#define S2D_ERR_UNSUPPORTED (-2)
#define S2D_ERR_CAPACITY (-3)
#define S2D_ERR_WORKSPACE (-4)
#define S2D_ERR_COMM (-5)

/* ---- library ------------------------------------------------------------------------------ */
/* 101: s2d_spconv_s16_sorted_supported / s2d_spconv_s16_fwd_sorted no longer take 64 -> 64 layers (128 -> 128 only); 100 before */
int s2d_version(void);
/* copies the calling thread's last error text (NUL terminated) into buf; returns its length */
int s2d_last_error(char *buf, size_t buf_len);
/* copies "compiler; HIP runtime headers; target; build date" of this library into buf; returns the text's length (no reference
 * counterpart: the reference's kernels come prebuilt with spconv / torch, docs/INSTALL.md:12,65-72) */
int s2d_build_info(char *buf, size_t buf_len);

/* ---- voxelization (hard voxelizer + fused reader mean) ------------------------------------ */
/*
 * Batched form: `frames` point clouds concatenated frame after frame (point_offsets[frames + 1], HOST array, offsets[0] = 0),
 * voxelized in ONE launch chain into the COLLATED example (preprocess.py:316-345 per frame + collate.py:105-144): voxels / num_points /
 * mean rows frame by frame in first-seen order, coors4[row] = (b, z, y, x) with the batch index prepended, out_m[frames] = voxels
 * per frame (device), out_base[frames + 1] = their exclusive prefix (out_base[frames] = total rows).  Outputs must hold
 * sum_b min(n_b, max_voxels) rows.  Same per-frame results as s2d_voxelize_run (bit exact).  frames <= 64.
 */
size_t s2d_voxelize_batch_workspace_bytes(int frames, const int64_t *point_offsets, int max_points, int max_voxels);
int s2d_voxelize_batch_run(const float *points, int frames, const int64_t *point_offsets, int ndim,
                           const float coors_range[6], const float voxel_size[3], int max_points, int max_voxels,
                           float *voxels, int32_t *coors4, int32_t *num_points, float *mean, int32_t *out_m,
                           int32_t *out_base, void *ws, size_t ws_bytes, s2d_stream_t stream);
/* workspace bytes for one call (hash table, per-point slots, scan scratch, k-smallest lists) */
size_t s2d_voxelize_workspace_bytes(int64_t n_points, int max_points, int max_voxels);
/*
 * points[n_points][ndim] fp32 (x,y,z,...) ; coors_range = xmin,ymin,zmin,xmax,ymax,zmax ;
 * voxel_size = (vx,vy,vz).  Outputs (rows >= *out_m are left untouched):
 *   voxels[max_voxels][max_points][ndim] fp32 (zero padded), coors[max_voxels][3] int32 (z,y,x),
 *   num_points[max_voxels] int32, mean[max_voxels][ndim] fp32 (may be NULL), out_m device int32.
 * Voxel order = order of first appearance in `points`; slot order = point order; voxels whose
 * first point comes after the max_voxels-th distinct voxel are dropped (reference semantics).
 */
int s2d_voxelize_run(const float *points, int64_t n_points, int ndim, const float coors_range[6],
                     const float voxel_size[3], int max_points, int max_voxels, float *voxels,
                     int32_t *coors, int32_t *num_points, float *mean, int32_t *out_m, void *ws,
                     size_t ws_bytes, s2d_stream_t stream);

/* ---- rulebooks ---------------------------------------------------------------------------- */
/*
 * A rulebook is a pair of dense gather maps (K = kD*kH*kW offsets, row-major over kz,ky,kx):
 *   nbr_out[k][o] = input row j feeding output row o through offset k, or -1
 *   nbr_in [k][j] = output row o fed by input row j through offset k, or -1   (transposed map,
 *                   used by the data-gradient; for SubM it is nbr_out[K-1-k] and not stored)
 * pair_count[k] = number of (j -> o) pairs of offset k (what spconv calls indice_pair_num).
 * `shape` is the (D,H,W) extent the coordinates index; coors rows are (b,z,y,x).
 */
size_t s2d_rulebook_workspace_bytes(int batch, const int32_t shape[3], int64_t n_rows);

/* SubM: output rows = input rows, same order; centred (pad = k/2, stride 1). */
int s2d_rulebook_subm_build(const int32_t *coors, int64_t n, int batch, const int32_t shape[3],
                            const int32_t ksize[3], const int32_t dilation[3], int32_t *nbr_out,
                            int32_t *pair_count, void *ws, size_t ws_bytes, s2d_stream_t stream);

/*
 * Regular (strided) conv, two phases around the one host read of *out_n:
 *   _count: marks every reachable output site, numbers them in sorted linear (b,z,y,x) order and
 *           writes the count to the device scalar out_n (workspace keeps the occupancy index);
 *   _fill : with n_out = *out_n known to the host, writes out_coors[n_out][4], nbr_out[K][n_out],
 *           nbr_in[K][n] and pair_count[K].  Must reuse the same workspace, unchanged.
 */
int s2d_rulebook_conv_count(const int32_t *coors, int64_t n, int batch, const int32_t shape[3],
                            const int32_t ksize[3], const int32_t stride[3],
                            const int32_t padding[3], const int32_t dilation[3], int32_t *out_n,
                            void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_rulebook_conv_fill(const int32_t *coors, int64_t n, int batch, const int32_t shape[3],
                           const int32_t ksize[3], const int32_t stride[3],
                           const int32_t padding[3], const int32_t dilation[3], int64_t n_out,
                           int32_t *out_coors, int32_t *nbr_out, int32_t *nbr_in,
                           int32_t *pair_count, void *ws, size_t ws_bytes, s2d_stream_t stream);

/*
 * r04 - every rulebook of one backbone pass in one chain (spconv get_indice_pairs x 8 as called by
 * det3d/models/backbones/scn.py:104-152: conv_input/conv1 .. conv4 SubM keys res0..res3 + the four strided convs).
 * Stage 0 = the input rows (any order); stage l+1 = outputs of strided conv l (ksize/stride/padding are [n_strided][3],
 * dilation 1, the first conv must be k3 s2 p1: its outputs index the 2x2x2 blocks of stage 0).
 *   _plan : marks + numbers the sites of stages 1..n (canonical sorted (b,z,y,x) order) and writes their row counts to the
 *           device vector counts[n_strided + 1] (last element: non-zero = internal error).  ONE host read per pass.
 *   _fill : with the counts known to the host (n_rows[n_strided]) writes out_coors[l] (stage l+1 rows), subm_nbr[l]
 *           (i32[27][N_l], l = 0..n_strided, NULL = not wanted), conv_nbr_out[l] (i32[K_l][N_{l+1}]), conv_nbr_in[l]
 *           (i32[K_l][N_l]) and pair_counts (i32[(2 n_strided + 1)][27]: SubM of stage l in row l, conv l in row
 *           n_strided + 1 + l).  `child` = scratch i32[n_rows[0]][8].  Same workspace as _plan, unchanged in between.
 * Maps are dense gather maps as above; every pointer array lives on the HOST and holds device pointers.
 */
int s2d_rulebook_chain_supported(int batch, const int32_t shape0[3], int n_strided, const int32_t *ksize,
                                 const int32_t *stride, const int32_t *padding);
size_t s2d_rulebook_chain_workspace_bytes(int batch, const int32_t shape0[3], int n_strided, const int32_t *ksize,
                                          const int32_t *stride, const int32_t *padding);
int s2d_rulebook_chain_plan(const int32_t *coors0, int64_t n0, int batch, const int32_t shape0[3], int n_strided,
                            const int32_t *ksize, const int32_t *stride, const int32_t *padding, int32_t *counts,
                            void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_rulebook_chain_fill(const int32_t *coors0, int64_t n0, int batch, const int32_t shape0[3], int n_strided,
                            const int32_t *ksize, const int32_t *stride, const int32_t *padding, const int64_t *n_rows,
                            int32_t *const *out_coors, int32_t *const *subm_nbr, int32_t *const *conv_nbr_out,
                            int32_t *const *conv_nbr_in, int32_t *pair_counts, int32_t *child, void *ws, size_t ws_bytes,
                            s2d_stream_t stream);

/* ---- sparse convolution (implicit GEMM on MFMA) ------------------------------------------- */
/*
 * out[o][:] = sum_k in[nbr[k][o]][:] * weight[k][:][:] (+ bias), fp32 in / fp32 accumulate on
 * v_mfma_f32_16x16x4_f32.  weight is [K][cin][cout] (spconv v1.x layout [kD,kH,kW,Cin,Cout]).
 * The same entry computes the data gradient when given nbr_in and the transposed weights.
 * `nbr` has row stride n_out.
 */
int s2d_spconv_fwd_f32(const float *in_feat, int64_t n_in, const float *weight, const float *bias,
                       const int32_t *nbr, int64_t n_out, int kvol, int cin, int cout,
                       float *out_feat, s2d_stream_t stream);
/*
 * bf16-input / fp32-accumulate variant (v_mfma_f32_16x16x32_bf16).  Features and outputs stay
 * fp32 in HBM; gathered rows are rounded to bf16 (RNE) in registers.  The weights are packed once
 * per call into the LDS image the kernel stages linearly (kvol*cin*cout bf16 = 2 bytes each).
 * Supported: cin in {32,64,128}, cout in {16,32,64,128} (s2d_spconv_bf16_supported).
 */
int s2d_spconv_bf16_supported(int cin, int cout);
/* (cin, cout) describe the packed operand.  transpose=1: `weight` is stored [K][cout][cin] (the
 * data gradient multiplies by W^T); flip=1: offsets mirrored, k -> K-1-k (SubM transposed map). */
int s2d_spconv_pack_weights_bf16(const float *weight, int kvol, int cin, int cout, int transpose,
                                 int flip, void *packed, s2d_stream_t stream);
int s2d_spconv_fwd_bf16(const float *in_feat, int64_t n_in, const void *packed_weight,
                        const float *bias, const int32_t *nbr, int64_t n_out, int kvol, int cin,
                        int cout, float *out_feat, s2d_stream_t stream);
/* dweight[k] = sum_o in[nbr[k][o]]^T * dout[o]  ([K][cin][cout]); deterministic two-pass. */
size_t s2d_spconv_wgrad_workspace_bytes(int64_t n_out, int kvol, int cin, int cout);
int s2d_spconv_wgrad_f32(const float *in_feat, int64_t n_in, const float *dout, const int32_t *nbr,
                         int64_t n_out, int kvol, int cin, int cout, float *dweight, void *ws,
                         size_t ws_bytes, s2d_stream_t stream);
/* The launch plan of a weight-gradient entry for these sizes, no device work (tests, tools): mode 0
 * s2d_spconv_wgrad_f32, 1 s2d_spconv_wgrad_bf16, 2 s2d_spconv_s16_wgrad.  out = {kernel, n_split,
 * rows_per_split, grid_y, wrow}; kernel 0 fp32 MFMA, 1 bf16 MFMA with register-assembled fragments,
 * 2 bf16 transpose-read, 3 workgroup-cooperative 128-channel, 4 VALU.  The plan, and with it the
 * workspace query above, follows S2D_WGRAD_TR / S2D_WGRAD_COOP / S2D_WGRAD_WAVES, which are read on
 * every call. */
int s2d_spconv_wgrad_plan(int mode, int64_t n_out, int kvol, int cin, int cout, int32_t out[5]);

/* same contract, MFMA inputs rounded to bf16 (fp32 accumulate); channel counts that the matrix path
 * does not cover fall back to the fp32 kernels inside. */
int s2d_spconv_wgrad_bf16(const float *in_feat, int64_t n_in, const float *dout, const int32_t *nbr,
                          int64_t n_out, int kvol, int cin, int cout, float *dweight, void *ws,
                          size_t ws_bytes, s2d_stream_t stream);

/* ---- BatchNorm1d on features (+ReLU, +residual) ------------------------------------------- */
/* stats[0..C) = sum_x, stats[C..2C) = sum_x^2 over the n rows (deterministic tree reduction) */
size_t s2d_bn1d_workspace_bytes(int64_t n, int c);
int s2d_bn1d_stats_f32(const float *x, int64_t n, int c, float *stats, void *ws, size_t ws_bytes,
                       s2d_stream_t stream);
/*
 * Per-channel finalisation, one launch each (replaces ~15 elementwise kernels per BN layer):
 *  fwd: stats[2C] and the (possibly all-reduced) row count -> mean, invstd, scale = gamma*invstd,
 *       shift = beta - mean*scale; running_mean/var (may both be NULL) updated with `momentum`
 *       and the unbiased variance, exactly like nn.BatchNorm1d.
 *  bwd: sums_local (this rank) and sums_global (all ranks; same pointer on one GPU) of
 *       [sum g, sum g*x] -> dgamma, dbeta (local, DDP averages them) and the three vectors of
 *       s2d_bn1d_bwd_apply_f32 (global).
 */
int s2d_bn1d_finalize_fwd_f32(const float *stats, const float *count, const float *gamma,
                              const float *beta, float eps, float momentum, int c, float *mean,
                              float *invstd, float *scale, float *shift, float *running_mean,
                              float *running_var, int64_t *batches_tracked, s2d_stream_t stream);
int s2d_bn1d_finalize_bwd_f32(const float *sums_local, const float *sums_global, const float *count,
                              const float *gamma, const float *mean, const float *invstd, int c,
                              float *dgamma, float *dbeta, float *a, float *b, float *d,
                              s2d_stream_t stream);
/* single-GPU fusions of {stats, finalize_fwd} and {bwd_reduce, finalize_bwd}: two launches each,
 * no intermediate [2C] vector on the host side (the multi-rank path keeps the split entries so the
 * sums can be all-reduced in between). */
int s2d_bn1d_stats_finalize_f32(const float *x, int64_t n, int c, const float *gamma,
                                const float *beta, float eps, float momentum, float *mean,
                                float *invstd, float *scale, float *shift, float *running_mean,
                                float *running_var, int64_t *batches_tracked, void *ws,
                                size_t ws_bytes, s2d_stream_t stream);
int s2d_bn1d_bwd_reduce_finalize_f32(const float *dy, const float *y, const float *x, int relu,
                                     int64_t n, int c, const float *gamma, const float *mean,
                                     const float *invstd, float *g_out, float *dgamma, float *dbeta,
                                     float *a, float *b, float *d, void *ws, size_t ws_bytes,
                                     s2d_stream_t stream);
/* y = relu?( (x - mean) * invstd * gamma + beta (+ residual) ); scale/shift precomputed [C] */
int s2d_bn1d_apply_f32(const float *x, const float *scale, const float *shift,
                       const float *residual, int relu, int64_t n, int c, float *y,
                       s2d_stream_t stream);
/*
 * Backward of y = relu?(x*scale + shift (+res)):  g = dy * (y > 0 if relu);
 * sums[0..C) = sum g, sums[C..2C) = sum g * x  (for dgamma/dbeta and the batch-stat terms);
 * g is written to dres (may alias nothing; may be NULL when there is no residual and dx is
 * produced by the second call).
 */
int s2d_bn1d_bwd_reduce_f32(const float *dy, const float *y, const float *x, int relu, int64_t n,
                            int c, float *g_out, float *sums, void *ws, size_t ws_bytes,
                            s2d_stream_t stream);
/* dx = a[c]*g + b[c]*x + d[c]  (training-mode BN backward folded into three per-channel vectors) */
int s2d_bn1d_bwd_apply_f32(const float *g, const float *x, const float *a, const float *b,
                           const float *d, int64_t n, int c, float *dx, s2d_stream_t stream);

/* ---- densify (SparseConvTensor.dense()) --------------------------------------------------- */
/* out[B][C][D][H][W] (zero filled here) <- features[n][C] at coors[n][4]; bwd is the gather. */
int s2d_densify_fwd_f32(const float *feat, const int32_t *coors, int64_t n, int batch,
                        const int32_t shape[3], int c, float *out, s2d_stream_t stream);
int s2d_densify_bwd_f32(const float *dout, const int32_t *coors, int64_t n, int batch,
                        const int32_t shape[3], int c, float *dfeat, s2d_stream_t stream);
/* dense() + view(N, C*D, H, W) written directly in the layout the bf16 BEV neck consumes:
 * out / dout are [batch][H][W][c*D] bf16 (torch channels_last of [batch][c*D][H][W]), BEV channel
 * = ch*D + z (scn.py:173-176).  feat / dfeat are [n][c], fp32 or (feat_bf16=1) bf16. */
int s2d_densify_bev_fwd_bf16(const void *feat, int feat_bf16, const int32_t *coors, int64_t n,
                             int batch, const int32_t shape[3], int c, void *out,
                             s2d_stream_t stream);
int s2d_densify_bev_bwd_bf16(const void *dout, const int32_t *coors, int64_t n, int batch,
                             const int32_t shape[3], int c, void *dfeat, int feat_bf16,
                             s2d_stream_t stream);

/* ---- PCR head of the S2D neck (dense, NCDHW fp32, HBM-bound) -------------------------------- */
/*
 * 1x1x1 convolution = per-position channel mixing (nn.Conv3d(k=1) / nn.Conv2d(k=1),
 * det3d/models/necks/rpn.py:263-296): out[n][co][p] = bias[co] + sum_ci weight[co][ci]*in[n][ci][p].
 * The data gradient is the same entry with the transposed weight and bias = NULL.
 */
int s2d_pointwise_conv_f32(const float *in, const float *weight, const float *bias, int batch,
                           int cin, int cout, int64_t positions, float *out, s2d_stream_t stream);
/*
 * nn.ConvTranspose3d(kernel 4, stride 2, padding 1) (rpn.py:267,284): in [n][cin][d][h][w] ->
 * out [n][cout][2d][2h][2w]; weight [cin][cout][4][4][4].  _dgrad is its input gradient.
 */
int s2d_convt3d_k4s2p1_fwd_f32(const float *in, const float *weight, const float *bias, int batch,
                               int cin, int cout, int d, int h, int w, float *out,
                               s2d_stream_t stream);
int s2d_convt3d_k4s2p1_dgrad_f32(const float *dout, const float *weight, int batch, int cin,
                                 int cout, int d, int h, int w, float *din, s2d_stream_t stream);
/* weight gradient [cin][cout][4][4][4] (cin, cout <= 32), fp32 matrix cores, deterministic */
size_t s2d_convt3d_k4s2p1_wgrad_workspace_bytes(int batch, int cin, int cout, int d, int h, int w);
int s2d_convt3d_k4s2p1_wgrad_f32(const float *in, const float *dout, int batch, int cin, int cout,
                                 int d, int h, int w, float *dweight, void *ws, size_t ws_bytes,
                                 s2d_stream_t stream);

/*
 * Channel-major batch norm (nn.BatchNorm3d / BatchNorm2d on NC[D]HW fp32 with few channels and
 * ~1e7 positions per plane: the PCR head, rpn.py:266-289).  Same maths and the same per-channel
 * finalisation entries as the row-major s2d_bn1d_* family; positions per plane must be a
 * multiple of 4.  stats/sums are [2C]: (sum x, sum x^2) resp. (sum g, sum g*x), g = dy*(y>0 if relu).
 */
size_t s2d_bncm_workspace_bytes(int batch, int c, int64_t positions);
int s2d_bncm_stats_f32(const float *x, int batch, int c, int64_t positions, float *stats, void *ws,
                       size_t ws_bytes, s2d_stream_t stream);
int s2d_bncm_apply_f32(const float *x, const float *scale, const float *shift, int relu, int batch,
                       int c, int64_t positions, float *y, s2d_stream_t stream);
int s2d_bncm_bwd_reduce_f32(const float *dy, const float *y, const float *x, int relu, int batch,
                            int c, int64_t positions, float *sums, void *ws, size_t ws_bytes,
                            s2d_stream_t stream);
int s2d_bncm_bwd_apply_f32(const float *dy, const float *y, const float *x, const float *a,
                           const float *b, const float *d, int relu, int batch, int c,
                           int64_t positions, float *dx, s2d_stream_t stream);
/* the two backward passes with the ReLU mask re-derived from x - y > 0 <=> fma(x, scale[c], shift[c]) > 0, the expression
 * s2d_bncm_apply_f32 evaluated, hence the same mask bit for bit - instead of reading the output planes a third time */
int s2d_bncm_bwd_reduce_x_f32(const float *dy, const float *x, const float *scale, const float *shift, int batch, int c, int64_t positions,
                              float *sums, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_bncm_bwd_apply_x_f32(const float *dy, const float *x, const float *scale, const float *shift, const float *a, const float *b,
                             const float *d, int batch, int c, int64_t positions, float *dx, s2d_stream_t stream);

/*
 * Dense 3x3 convolution, stride 1 (or 2: forward only), padding 0 or 1, on NHWC bf16 activations (the BEV neck blocks
 * and the CenterHead towers: det3d/models/necks/rpn.py:126-145, bbox_heads/center_head.py:209-232;
 * replaces the cuDNN call behind nn.Conv2d there).  Implicit GEMM on v_mfma_f32_16x16x32_bf16,
 * fp32 accumulate, bf16 output [N][Ho][Wo][cout].  cin and cout multiples of 64.
 * The weight ([cout][cin][3][3] fp32, torch layout) is packed once per call into the kernel's
 * LDS image (9*cin*cout bf16).  transpose_flip=1 packs the data-gradient operand: then (cin,cout)
 * = (forward cout, forward cin) and the forward kernel run on dY with pad 1 yields dX (a pad-0
 * forward first pads dY by one ring of zeros).  weight_nhwc=1: `weight` memory order is
 * [cout][3][3][cin] (torch channels_last).  zero_page: >= 16 zero bytes of device memory
 * (source of the border taps).
 */
int s2d_conv2d3x3_supported(int cin, int cout);
int s2d_conv2d3x3_pack_weights_bf16(const float *weight, int cin, int cout, int transpose_flip,
                                    int weight_nhwc, void *packed, s2d_stream_t stream);
/* stats_partial (optional, fp32 [tiles][2][cout], tiles = s2d_conv2d3x3_stats_tiles(...) for the same shape - the
 * pixel-tile height is chosen per launch): per pixel tile (sum, sum of squares) of the stored
 * outputs per channel — the statistics pass of a following batch norm, produced in the conv epilogue; finish it with
 * s2d_bn_partials_finalize_f32 (or s2d_bn_partials_sum_f32 -> all-reduce -> s2d_bn1d_finalize_fwd_f32). */
int64_t s2d_conv2d3x3_stats_tiles(int n_img, int h, int w, int cin, int cout, int pad, int stride);
/* output pixels per workgroup tile of the launch plan for this shape (= rows per BN-statistics slab) */
int s2d_conv2d3x3_tile_rows(int n_img, int h, int w, int cin, int cout, int pad, int stride);
int s2d_conv2d3x3_nhwc_bf16(const void *x, const void *packed_weight, const float *bias,
                            const void *zero_page, int n_img, int h, int w, int cin, int cout,
                            int pad, int stride, void *y, float *stats_partial, s2d_stream_t stream);
/* batch-norm statistics from per-tile partial sums [nblocks][2][c] (a conv epilogue's stats_partial) over n rows:
 * fused finalize (mean, invstd, scale, shift, running stats, batches_tracked) or the plain [2c](+count) sums */
int s2d_bn_partials_finalize_f32(const float *partial, int nblocks, int64_t n, int c, const float *gamma,
                                 const float *beta, float eps, float momentum, float *mean,
                                 float *invstd, float *scale, float *shift, float *running_mean,
                                 float *running_var, int64_t *batches_tracked, s2d_stream_t stream);
int s2d_bn_partials_sum_f32(const float *partial, int nblocks, int64_t n, int c, float *stats,
                            int write_count, s2d_stream_t stream);
/* the same with a workspace (s2d_bn_partials_sum_workspace_bytes, 0 = not needed): lists of more than 1536 rows (a producer that
 * writes one row per tile, e.g. s2d_convt3d_mfma_fwd_stats) are folded in two stages, fixed order */
size_t s2d_bn_partials_sum_workspace_bytes(int nblocks, int c);
int s2d_bn_partials_sum_ws_f32(const float *partial, int nblocks, int64_t n, int c, float *stats, int write_count, void *ws,
                               size_t ws_bytes, s2d_stream_t stream);
/* s2d_bn_partials_finalize_f32 with the same optional workspace (two-stage fold of lists longer than 1536 rows) */
int s2d_bn_partials_finalize_ws_f32(const float *partial, int nblocks, int64_t n, int c, const float *gamma, const float *beta, float eps,
                                    float momentum, float *mean, float *invstd, float *scale, float *shift, float *running_mean,
                                    float *running_var, int64_t *batches_tracked, void *ws, size_t ws_bytes, s2d_stream_t stream);

/* Batch-norm backward sums out of the data-gradient conv (r06; rpn.py:126-145 conv -> BatchNorm2d -> ReLU chains, rpn.py:186-253
 * conv -> BatchNorm2d -> GELU groups; replaces the reduction half of the cuDNN batch-norm backward there).  When the conv being
 * differentiated reads the output of y = act(z * scale + shift) (act: 0 none, 1 ReLU, 2 exact GELU), its data gradient IS that layer's
 * dY: the *_bnbwd forms of the conv entries take z (bf16 [n][h][w][cout of this launch]) and the layer's fp32 scale / shift and write,
 * next to dY, the per-tile sums (sum g, sum g z), g = dY act'(z scale + shift) over the stored bf16 dY, to bn_partial[tiles][2][cout]
 * (tiles = s2d_conv2d3x3_stats_tiles / s2d_conv2d1x1_stats_tiles of the same launch shape).  s2d_bn_partials_bwd_finalize_ws_f32 folds
 * them (fixed order) into dgamma, dbeta and the coefficients a, b, d of s2d_bnrow_bwd_apply_ld_bf16 - no pass over (dY, z) in between.
 * *_supported: the launch plan of the shape takes the kernel that carries the epilogue (stride 1). */
int s2d_conv2d3x3_bnbwd_supported(int cin, int cout, int pad, int stride);
int s2d_conv2d3x3_nhwc_bf16_bnbwd(const void *x, const void *packed_weight, const void *zero_page, int n_img, int h, int w, int cin, int cout,
                                  int pad, void *y, const void *bn_z, const float *bn_scale, const float *bn_shift, int bn_act,
                                  float *bn_partial, s2d_stream_t stream);
int s2d_conv2d1x1_bnbwd_supported(int cin, int cout);
int s2d_conv2d1x1_nhwc_bf16_bnbwd(const void *x, const void *packed_weight, const void *zero_page, int n_img, int h, int w, int cin, int cout,
                                  void *y, const void *bn_z, const float *bn_scale, const float *bn_shift, int bn_act, float *bn_partial,
                                  s2d_stream_t stream);
int s2d_bn_partials_bwd_finalize_ws_f32(const float *partial, int nblocks, int64_t n, int c, const float *gamma, const float *mean,
                                        const float *invstd, float *dgamma, float *dbeta, float *a, float *b, float *d, void *ws,
                                        size_t ws_bytes, s2d_stream_t stream);

/*
 * Row-major bf16 batch norm: nn.BatchNorm2d (+ the ReLU that follows it) on NHWC bf16 activations
 * viewed as [n = N*H*W rows][c] (BEV neck and head: rpn.py:126-145, center_head.py:209-232;
 * replaces the cuDNN batch-norm calls there).  c multiple of 8, <= 1024.  Statistics and all
 * per-channel vectors are fp32 and use the same finalisation as the s2d_bn1d_* family
 * (s2d_bn1d_finalize_fwd/bwd_f32 after an all-reduce of the split `stats` / `sums` vectors, or the
 * fused *_finalize entries on one GPU).  Also the batch norm of the bf16-storage sparse stack
 * ([n sites][c], scn.py:73-83) with `residual` added before the ReLU.  Backward: with y == NULL the
 * ReLU mask is recomputed from x, scale and shift (y > 0 <=> x*scale+shift > 0; only valid without a
 * residual), otherwise taken from y; dres (optional) receives the masked dy, i.e. the gradient of
 * the residual branch.  `relu` is an activation code: 0 none, 1 ReLU, 2 exact (erf) GELU - the conv-BN-GELU groups of the
 * S2D module (det3d/models/necks/rpn.py:186-253); the GELU derivative is always recomputed from x, scale and shift.
 */
size_t s2d_bnrow_workspace_bytes(int64_t n, int c);
/* stats: [2c] sums, plus the row count at stats[2c] when write_count (the [2c+1] vector SyncBN all-reduces) */
int s2d_bnrow_stats_bf16(const void *x, int64_t n, int c, float *stats, int write_count, void *ws,
                         size_t ws_bytes, s2d_stream_t stream);
int s2d_bnrow_stats_finalize_bf16(const void *x, int64_t n, int c, const float *gamma,
                                  const float *beta, float eps, float momentum, float *mean,
                                  float *invstd, float *scale, float *shift, float *running_mean,
                                  float *running_var, int64_t *batches_tracked, void *ws,
                                  size_t ws_bytes, s2d_stream_t stream);
int s2d_bnrow_apply_bf16(const void *x, const float *scale, const float *shift, const void *residual,
                         int relu, int64_t n, int c, void *y, s2d_stream_t stream);
/* sums_copy (optional): second copy of the [2c] sums — the local one feeds dgamma/dbeta, the copy is all-reduced */
int s2d_bnrow_bwd_reduce_bf16(const void *dy, const void *x, const void *y, const float *scale,
                              const float *shift, int relu, int64_t n, int c, float *sums,
                              float *sums_copy, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_bnrow_bwd_reduce_finalize_bf16(const void *dy, const void *x, const void *y,
                                       const float *scale, const float *shift, int relu, int64_t n, int c,
                                       const float *gamma, const float *mean, const float *invstd,
                                       float *dgamma, float *dbeta, float *a, float *b, float *d,
                                       void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_bnrow_bwd_apply_bf16(const void *dy, const void *x, const void *y, const float *scale,
                             const float *shift, int relu, const float *a, const float *b,
                             const float *d, int64_t n, int c, void *dx, void *dres,
                             s2d_stream_t stream);
/* Leading-dimension variants (r04): y / dy may be a channel slice of a wider row-major bf16 tensor - y_ld / dy_ld = its row stride in
 * elements (a multiple of 8, >= c; the pointer is the slice's first element).  Lets the RPN's up-sampling branches write their
 * batch-norm outputs straight into the concatenated tensor and read their gradients out of its gradient: no torch.cat copy, no
 * contiguous copies of the gradient slices (rpn.py:156-171). */
int s2d_bnrow_apply_ld_bf16(const void *x, const float *scale, const float *shift, const void *residual, int relu, int64_t n, int c, void *y,
                            int y_ld, s2d_stream_t stream);
int s2d_bnrow_bwd_reduce_ld_bf16(const void *dy, int dy_ld, const void *x, const void *y, const float *scale, const float *shift, int relu,
                                 int64_t n, int c, float *sums, float *sums_copy, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_bnrow_bwd_reduce_finalize_ld_bf16(const void *dy, int dy_ld, const void *x, const void *y, const float *scale, const float *shift,
                                          int relu, int64_t n, int c, const float *gamma, const float *mean, const float *invstd,
                                          float *dgamma, float *dbeta, float *a, float *b, float *d, void *ws, size_t ws_bytes,
                                          s2d_stream_t stream);
int s2d_bnrow_bwd_apply_ld_bf16(const void *dy, int dy_ld, const void *x, const void *y, const float *scale, const float *shift, int relu,
                                const float *a, const float *b, const float *d, int64_t n, int c, void *dx, void *dres,
                                s2d_stream_t stream);

/*
 * bf16-storage sparse convolution ("s16" path): features and outputs are bf16 [n][c] in HBM,
 * fp32 accumulation on v_mfma_f32_16x16x32_bf16.  Same gather-map contract as s2d_spconv_fwd_f32
 * (nbr[k][o] = input row feeding output row o through kernel offset k, or -1); the data gradient is
 * the same entry run on dout with nbr_in (or the SubM map with flip=1) and the weight image packed
 * with transpose=1.  cin, cout in {16, 32, 64, 128}.  Two kernels sit behind these entries: shapes with 128 input or output
 * channels (and >= 64 on the other side) run the register-gather kernel (csrc/spconv_rg.hip: A fragments gathered straight
 * into MFMA operand registers, weight slab through LDS), the others the LDS-staged kernel (csrc/spconv_s16.hip).  The weight
 * image depends on the kernel and its launch tiling chosen from n_out, so pack and fwd must be given the same n_out.
 * zero_page: >= 16 zero bytes of device memory (what a missing neighbour reads in the LDS-staged kernel).
 */
int s2d_spconv_s16_supported(int cin, int cout);
size_t s2d_spconv_s16_packed_elems(int kvol, int cin, int cout);
int s2d_spconv_s16_pack_weights(const float *weight, int kvol, int cin, int cout, int transpose,
                                int flip, int64_t n_out, void *packed, s2d_stream_t stream);
/* both operands of a layer in one launch (the weight changes once per optimizer step): packed_fwd as above for a forward launch over
 * n_out_fwd rows, packed_dgrad = the [cout -> cin] operand (transpose = 1, flip = flip_dgrad) for the data-gradient launch over n_out_dgrad rows */
int s2d_spconv_s16_pack_weights_pair(const float *weight, int kvol, int cin, int cout, int flip_dgrad, int64_t n_out_fwd, int64_t n_out_dgrad,
                                     void *packed_fwd, void *packed_dgrad, s2d_stream_t stream);
/* weight gradient of the s16 path (in_feat, dout bf16; dweight fp32 [kvol][cin][cout]); workspace from
 * s2d_spconv_wgrad_workspace_bytes */
int s2d_spconv_s16_wgrad(const void *in_feat, int64_t n_in, const void *dout, const int32_t *nbr,
                         int64_t n_out, int kvol, int cin, int cout, float *dweight, void *ws,
                         size_t ws_bytes, s2d_stream_t stream);
int s2d_spconv_s16_fwd(const void *in_feat, int64_t n_in, const void *packed_weight,
                       const float *bias, const int32_t *nbr, int64_t n_out, int kvol, int cin,
                       int cout, const void *zero_page, void *out_feat, s2d_stream_t stream);
/* the same with the batch-norm statistics of the layer that follows from the epilogue: stats_partial = fp32
 * [s2d_spconv_s16_stats_tiles(n_out, kvol, cin, cout)][2][cout], per-workgroup (sum, sum of squares) of the stored bf16 rows, folded by
 * s2d_bn_partials_finalize_f32 / s2d_bn_partials_sum_f32 (replaces the separate statistics pass of spconv's conv -> BatchNorm1d pairs,
 * /root/reference/det3d/models/backbones/scn.py:60-90) */
int64_t s2d_spconv_s16_stats_tiles(int64_t n_out, int kvol, int cin, int cout);
int s2d_spconv_s16_fwd_stats(const void *in_feat, int64_t n_in, const void *packed_weight, const float *bias, const int32_t *nbr,
                             int64_t n_out, int kvol, int cin, int cout, const void *zero_page, void *out_feat, float *stats_partial,
                             s2d_stream_t stream);

/*
 * r06 - rows of a submanifold rulebook grouped by neighbour mask, and the implicit GEMM over the grouped rows.
 * (spconv.ops.get_indice_pairs / indice_conv; call sites /root/reference/det3d/models/backbones/scn.py:104-152)
 * s2d_rulebook_sort_by_mask: from the dense gather map nbr [kvol][n] of a rulebook (kvol <= 27) builds
 *   pmask [n] u32   neighbour mask (bit k = offset k present) of the rows in ascending mask order per chunk (stable radix sort: deterministic),
 *   perm  [n] i32   canonical row index of each sorted position,
 *   nbr_perm [kvol][n] i32 = nbr[k][perm[j]].
 * s2d_spconv_s16_fwd_sorted: the bf16-storage sparse conv (same packed weight image as s2d_spconv_s16_fwd for the layer) over the sorted
 * rows: every workgroup multiplies only the kernel offsets present in the union of its rows' masks, every wave only those present in its
 * 16-row tile; results are stored to the canonical rows perm[j], so out_feat (and stats_partial: the same
 * [s2d_spconv_s16_stats_tiles][2][cout] layout) are what s2d_spconv_s16_fwd_stats returns, up to the summation order of the statistics.
 * Supported: kvol 27, 128 -> 128 channels (s2d_spconv_s16_sorted_supported).
 * OPT-IN: measured on the benchmark scene's rulebooks (profiles/r06_sparse_sorted_rows_ab.txt) the sorted form is 5-10 % SLOWER than the
 * plain kernel although it issues 37 % fewer MFMAs - the kernel is bound by the gathered rows, which skipping does not reduce.
 * s2d_spconv_s16_set_sorted_rows(1) (or S2D_RG_SORTED=1 in the environment) switches it on and returns the previous setting.
 */
int s2d_spconv_s16_set_sorted_rows(int on);
size_t s2d_rulebook_sort_workspace_bytes(int64_t n);
/* the sort stays inside chunks of this many canonical rows (the rows one XCD's workgroups of the consuming kernel process): ascending masks
 * within a chunk, chunks in canonical order */
int64_t s2d_rulebook_sort_chunk_rows(int64_t n);
int s2d_rulebook_sort_by_mask(const int32_t *nbr, int kvol, int64_t n, int32_t *perm, uint32_t *pmask, int32_t *nbr_perm, void *ws,
                              size_t ws_bytes, s2d_stream_t stream);
int s2d_spconv_s16_sorted_supported(int kvol, int cin, int cout);
int s2d_spconv_s16_fwd_sorted(const void *in_feat, int64_t n_in, const void *packed_weight, const float *bias, const int32_t *nbr_perm,
                              const int32_t *perm, const uint32_t *pmask, int64_t n_out, int kvol, int cin, int cout, void *out_feat,
                              float *stats_partial, s2d_stream_t stream);

/*
 * Weight gradient of the dense 3x3 stride-1 convolution above (replaces the cuDNN backward-filter call):
 * x [n][h][w][cin] bf16 (the forward input), dy [n][ho][wo][cout] bf16, dweight fp32 in the torch layout
 * [cout][cin][3][3].  cin, cout multiples of 64.  Pixels are contracted on v_mfma_f32_16x16x32_bf16 through LDS
 * transpose reads; split partial sums are reduced in a fixed order (deterministic).
 */
int s2d_conv2d3x3_wgrad_supported(int cin, int cout);
size_t s2d_conv2d3x3_wgrad_workspace_bytes(int n_img, int h, int w, int cin, int cout, int pad);
int s2d_conv2d3x3_wgrad_nhwc_bf16(const void *x, const void *dy, const void *zero_page, int n_img,
                                  int h, int w, int cin, int cout, int pad, float *dweight, float *dbias /* [cout] or NULL: per-channel
                                  sums of dy = nn.Conv2d's bias gradient, accumulated by the same launch */, void *ws,
                                  size_t ws_bytes, s2d_stream_t stream);

/*
 * 1x1 convolutions (stride 1) of the S2D module (det3d/models/necks/rpn.py:186-253: fusion_sparse / fusion_dense, out_conv, the ConvNeXt
 * point-wise pairs) on NHWC bf16: GEMMs over the pixel rows on the same tile pipeline, weight image and epilogue (bias, per-tile
 * batch-norm statistics [tiles][2][cout], tiles = s2d_conv2d1x1_stats_tiles) as the 3x3 kernels.  pack: weight = torch
 * [Cout][Cin][1][1] of the forward conv, (cin, cout) = dimensions of the packed operand, transpose = 1 for the data gradient (run the
 * forward entry on dY).  Channels: multiples of 64.
 */
int s2d_conv2d1x1_pack_weights_bf16(const float *weight, int cin, int cout, int transpose, void *packed, s2d_stream_t stream);
/* both operands of a layer in one launch (the weight changes once per optimizer step, every training step needs both): weight = torch
 * [cout][cin][k][k] of the forward conv; packed_fwd = its [cin -> cout] image, packed_dgrad = the [cout -> cin] image with mirrored taps */
int s2d_conv2d3x3_pack_weights_pair_bf16(const float *weight, int cin, int cout, int weight_nhwc, void *packed_fwd, void *packed_dgrad,
                                         s2d_stream_t stream);
int s2d_conv2d1x1_pack_weights_pair_bf16(const float *weight, int cin, int cout, void *packed_fwd, void *packed_dgrad, s2d_stream_t stream);
int64_t s2d_conv2d1x1_stats_tiles(int n_img, int h, int w, int cin, int cout);
int s2d_conv2d1x1_nhwc_bf16(const void *x, const void *packed_weight, const float *bias, const void *zero_page, int n_img,
                            int h, int w, int cin, int cout, void *y, float *stats_partial, s2d_stream_t stream);
size_t s2d_conv2d1x1_wgrad_workspace_bytes(int n_img, int h, int w, int cin, int cout);
int s2d_conv2d1x1_wgrad_nhwc_bf16(const void *x, const void *dy, const void *zero_page, int n_img, int h, int w, int cin,
                                  int cout, float *dweight, float *dbias /* [cout] or NULL */, void *ws, size_t ws_bytes, s2d_stream_t stream);

/* 3x3 / padding 1 / stride 1 convolutions with 1..4 output channels: the last conv of every CenterHead branch
 * (/root/reference/det3d/models/bbox_heads/center_head.py:33-61 SepHead, Conv2d(64, classes, 3, padding=1); replaces the
 * torch.nn.Conv2d -> MIOpen call there).  x, dx: bf16 NHWC [n][h][w][cin] (cin in {8,16,32,64,128}); weight / dweight: fp32
 * [cout][cin][3][3] (torch layout); y, dy: fp32 planar [n][cout][h][w] - the predictions the losses and the decoder read.
 * wgrad also returns dbias (optional); its per-block partial sums are folded in a fixed order (deterministic). */
int s2d_smallconv3x3_supported(int cin, int cout);
int s2d_smallconv3x3_fwd(const void *x, const float *weight, const float *bias, int n_img, int h, int w, int cin, int cout, float *y,
                         s2d_stream_t stream);
int s2d_smallconv3x3_dgrad(const float *dy, const float *weight, int n_img, int h, int w, int cin, int cout, void *dx,
                           s2d_stream_t stream);
size_t s2d_smallconv3x3_wgrad_workspace_bytes(int cin, int cout);
int s2d_smallconv3x3_wgrad(const void *x, const float *dy, int n_img, int h, int w, int cin, int cout, float *dweight, float *dbias,
                           void *ws, size_t ws_bytes, s2d_stream_t stream);

/*
 * 2x2 stride-2 convolution forward (encoder_1[0] of the S2D module, rpn.py:188) on the same tile pipeline; weight = torch
 * [Cout][Cin][2][2] (weight_nhwc = 1: channels_last memory), output [n][h/2][w/2][cout], optional BN-statistics slabs.
 */
int s2d_conv2d2x2s2_pack_weights_bf16(const float *weight, int cin, int cout, int weight_nhwc, void *packed, s2d_stream_t stream);
int64_t s2d_conv2d2x2s2_stats_tiles(int n_img, int h, int w);
int s2d_conv2d2x2s2_nhwc_bf16(const void *x, const void *packed_weight, const float *bias, const void *zero_page, int n_img,
                              int h, int w, int cin, int cout, void *y, float *stats_partial, s2d_stream_t stream);

/*
 * Stride-2 transposed convolutions and their gradients on the same tile pipeline (replace the MIOpen calls behind
 * nn.ConvTranspose2d(256, 256, 4, 2, 1) in decoder_1 / decoder_2 of the S2D module, det3d/models/necks/rpn.py:217-231, and behind
 * the backward of the RPN's stride-2 3x3 convs, rpn.py:126-133).
 *   convup (ks = 4): ConvTranspose2d(4,2,1) forward, x [n][h][w][kc] -> y [n][2h][2w][nc], weight fp32 [kc][nc][4][4] (torch layout),
 *          optional bias and BN-statistics slabs [s2d_convup_stats_tiles][2][nc];
 *   convup (ks = 3): data gradient of Conv2d(nc -> kc, 3, stride 2, pad 1): dY [n][h][w][kc] -> dX [n][2h][2w][nc], weight [kc][nc][3][3];
 *   conv2d4x4s2: Conv2d(cin -> cout, 4, stride 2, pad 1) = data gradient of ConvTranspose2d(cout -> cin, 4,2,1); weight fp32
 *          [cout][cin][4][4] in the forward-conv sense = the transposed conv's weight as stored; x [n][h][w][cin] -> [n][h/2][w/2][cout];
 *   conv2d_s2_wgrad: dW[ca][cb][ks][ks] = sum a[n][i][j][.] * b[n][2i-1+ky][2j-1+kx][.] with a [n][h/2][w/2][ca], b [n][h][w][cb]
 *          (ConvTranspose2d: a = input, b = dY; stride-2 conv: a = dY, b = input); fixed-order split reduction in ws.
 */
int s2d_convup_supported(int kc, int nc, int ks);
int s2d_convup_pack_weights_bf16(const float *weight, int kc, int nc, int ks, void *packed, s2d_stream_t stream);
int64_t s2d_convup_stats_tiles(int n_img, int h, int w, int kc, int nc, int ks);
int s2d_convup_nhwc_bf16(const void *x, const void *packed_weight, const float *bias, const void *zero_page, int n_img, int h, int w,
                         int kc, int nc, int ks, void *y, float *stats_partial, s2d_stream_t stream);
int s2d_conv2d4x4s2_pack_weights_bf16(const float *weight, int cin, int cout, void *packed, s2d_stream_t stream);
int s2d_conv2d4x4s2_nhwc_bf16(const void *x, const void *packed_weight, const void *zero_page, int n_img, int h, int w, int cin,
                              int cout, void *y, s2d_stream_t stream);
int s2d_conv2d_s2_wgrad_supported(int ca, int cb, int ks);
size_t s2d_conv2d_s2_wgrad_workspace_bytes(int n_img, int h, int w, int ca, int cb, int ks);
int s2d_conv2d_s2_wgrad_nhwc_bf16(const void *a, const void *b, const void *zero_page, int n_img, int h, int w, int ca, int cb, int ks,
                                  float *dweight, void *ws, size_t ws_bytes, s2d_stream_t stream);

/*
 * Weight gradient of a bias-free Linear over a long row-major fp32 matrix (PFNLayer.linear of the pillar reader,
 * det3d/models/readers/pillar_encoder.py:41-56; replaces the GEMM behind torch.mm in nn.Linear's backward):
 *   dweight[co][ci] = sum_r dy[r][co] * x[r][ci];  x [rows][ci], dy [rows][co]; ci, co <= 64; exact fp32 (v_mfma_f32_16x16x4_f32),
 *   fixed-order split reduction in ws (s2d_rows_wgrad_workspace_bytes).
 */
int s2d_rows_wgrad_supported(int ci, int co);
size_t s2d_rows_wgrad_workspace_bytes(int64_t rows, int ci, int co);
int s2d_rows_wgrad_f32(const float *x, const float *dy, int64_t rows, int ci, int co, float *dweight, void *ws, size_t ws_bytes,
                       s2d_stream_t stream);

/*
 * Depth-wise 7x7 convolution, padding 3, stride 1 (nn.Conv2d(C, C, 7, padding=3, groups=C): first layer of the three
 * ConvNeXt blocks of the S2D module, det3d/models/necks/rpn.py:204-225) on NHWC bf16 maps.  x, y [n][h][w][c] bf16;
 * weight fp32 [c][49] (the torch layout [c][1][7][7]); bias fp32 [c] or NULL; fp32 accumulation.  flip=1 mirrors the taps:
 * the data gradient is the same stencil applied to dy.  c must be a multiple of 8.  The weight gradient returns dweight
 * fp32 [c][49] and (optionally) dbias [c]; its partial sums are folded in a fixed order (deterministic).
 */
int s2d_dwconv7_supported(int channels);
int s2d_dwconv7_nhwc_bf16(const void *x, const float *weight, const float *bias, int n_img, int h, int w,
                          int c, int flip, void *y, s2d_stream_t stream);
size_t s2d_dwconv7_wgrad_workspace_bytes(int n_img, int h, int w, int c);
int s2d_dwconv7_wgrad_nhwc_bf16(const void *x, const void *dy, int n_img, int h, int w, int c,
                                float *dweight, float *dbias, void *ws, size_t ws_bytes,
                                s2d_stream_t stream);

/*
 * ConvTranspose3d(kernel 4, stride 2, padding 1) of the PCR head on the bf16 matrix cores (bf16 compute mode;
 * det3d/models/necks/rpn.py:263-296: 32->32 and 16->3).  Tensors are NCDHW fp32 exactly as in s2d_convt3d_k4s2p1_*_f32;
 * activations and weights are rounded to bf16 while staged, accumulation is fp32.  cin in {16, 32}, cout <= 32.
 * `packed` = s2d_convt3d_mfma_packed_elems bf16 elements holding the forward and data-gradient weight images (rebuild it
 * whenever the weight changes).
 */
int s2d_convt3d_mfma_supported(int cin, int cout);
size_t s2d_convt3d_mfma_packed_elems(int cin, int cout);
int s2d_convt3d_mfma_pack_weights(const float *weight, int cin, int cout, void *packed, s2d_stream_t stream);
int s2d_convt3d_mfma_fwd(const float *in, const void *packed, const float *bias, int batch, int cin, int cout,
                         int d, int h, int w, float *out, s2d_stream_t stream);
/* ... with the statistics pass of the BatchNorm3d that follows folded into the epilogue: stats_partial (optional)
 * [s2d_convt3d_mfma_stats_tiles(batch,cin,d,h,w)][2][cout] = per-block (sum, sum of squares) per output channel of the written
 * output; s2d_bn_partials_sum_f32 folds them into the [2*cout] statistics vector */
int64_t s2d_convt3d_mfma_stats_tiles(int batch, int cin, int d, int h, int w);
int s2d_convt3d_mfma_fwd_stats(const float *in, const void *packed, const float *bias, int batch, int cin, int cout,
                               int d, int h, int w, float *out, float *stats_partial, s2d_stream_t stream);
int s2d_convt3d_mfma_dgrad(const float *dout, const void *packed, int batch, int cin, int cout, int d, int h,
                           int w, float *din, s2d_stream_t stream);
size_t s2d_convt3d_mfma_wgrad_workspace_bytes(int batch, int cin, int cout, int d, int h, int w);
int s2d_convt3d_mfma_wgrad(const float *in, const float *dout, int batch, int cin, int cout, int d, int h,
                           int w, float *dweight, void *ws, size_t ws_bytes, s2d_stream_t stream);
/* bf16-stored output gradient (r04): the same data / weight gradients from a dout the producer wrote in bf16 - the kernels above round
 * dout to bf16 on load, so the results are identical and the 0.5-0.7 GB tensor is half as large.  _supported: the layer shapes the
 * bf16-reading kernels cover (d, h, w = INPUT extents). */
int s2d_convt3d_mfma_d16_supported(int cin, int cout, int d, int h, int w);
int s2d_convt3d_mfma_dgrad_d16(const void *dout_bf16, const void *packed, int batch, int cin, int cout, int d, int h, int w, float *din,
                               s2d_stream_t stream);
int s2d_convt3d_mfma_wgrad_d16(const float *in, const void *dout_bf16, int batch, int cin, int cout, int d, int h, int w, float *dweight,
                               void *ws, size_t ws_bytes, s2d_stream_t stream);
/* The BatchNorm3d + ReLU in FRONT of the layer folded into its kernels (r04): `in` is the raw tensor, in_scale_shift = scale[cin] |
 * shift[cin] (device), applied as relu(fma(x, scale, shift)) - the expression of s2d_bncm_apply_f32 - while the forward stages its input
 * and while the weight gradient loads it; the normalised tensor is never written or read. */
int s2d_convt3d_mfma_norm_supported(int cin, int cout, int d, int h, int w);   /* the layers it pays on: narrow outputs (cout <= 4, w % 8 == 0) */
int s2d_convt3d_mfma_fwd_stats_y16_norm(const float *in, const float *in_scale_shift, const void *packed, const float *bias, int batch,
                                        int cin, int cout, int d, int h, int w, void *out_bf16, float *stats_partial, s2d_stream_t stream);
int s2d_convt3d_mfma_wgrad_d16_norm(const float *in, const float *in_scale_shift, const void *dout_bf16, int batch, int cin, int cout, int d,
                                    int h, int w, float *dweight, void *ws, size_t ws_bytes, s2d_stream_t stream);

/* weight (+ bias) gradient of the 1x1x1 Conv3d layers of the PCR head: dweight[cout][cin] = sum_{n,p} dout[n][co][p] in[n][ci][p],
 * dbias[cout] = sum dout (NCDHW fp32 tensors, positions % 4 == 0); deterministic two-stage reduction */
size_t s2d_pointwise_conv_wgrad_workspace_bytes(int cin, int cout);
int s2d_pointwise_conv_wgrad_f32(const float *in, const float *dout, int batch, int cin, int cout,
                                 int64_t positions, float *dweight, float *dbias, void *ws, size_t ws_bytes,
                                 s2d_stream_t stream);
/* same contract (and workspace) with both operands rounded to bf16 and contracted on the matrix cores in ONE pass over the two
 * tensors; supported: (cin 128, cout <= 32), (cin 32, cout <= 16), positions % 4 == 0, one sample's planes < 2 GB */
int s2d_pointwise_conv_wgrad_bf16_supported(int cin, int cout, int64_t positions);
int s2d_pointwise_conv_wgrad_bf16(const float *in, const float *dout, int batch, int cin, int cout,
                                 int64_t positions, float *dweight, float *dbias, void *ws, size_t ws_bytes,
                                 s2d_stream_t stream);
/* ... with x = relu(in*scale + shift) applied on the fly (the conv's input was a batch norm + ReLU of `in`):
 * in_scale_shift (device, 2*cin) = scale[cin] | shift[cin], NULL = plain */
int s2d_pointwise_conv_wgrad_norm_bf16(const float *in, const float *in_scale_shift, const float *dout, int batch,
                                       int cin, int cout, int64_t positions, float *dweight, float *dbias,
                                       void *ws, size_t ws_bytes, s2d_stream_t stream);

/*
 * PCR (point-cloud reconstruction) losses of the S2D student, det3d/models/detectors/voxelnet.py:171-185,203-249
 * (`mask_offset_loss` on the dense reconstruction target), computed from the SPARSE recon voxels instead of the dense
 * [B,5,D,H,W] target: gen_offset fp32 [B][3][D][H][W], gen_mask fp32 [B][1][D][H][W] (logits), coors int32 [m][4] (b,z,y,x)
 * and feats fp32 [m][5] = the reader output of the recon voxels at this scale.  out8 (device, 8 floats):
 * [0] mask_loss (BCE-with-logits, pos_weight = #neg/#pos, mean over all cells)  [1] offset_loss (L1 at the non-zero target
 * entries)  [2] beta  [3] n_sel  [4] N  [5] n_pos.  The backward takes out8 and the two upstream scalar gradients (device)
 * and writes d/d gen_mask (every cell) and d/d gen_offset (only the selected entries: the caller passes a zeroed buffer).
 */
size_t s2d_pcr_loss_workspace_bytes(void);
int s2d_pcr_loss_fwd_f32(const float *gen_offset, const float *gen_mask, const int32_t *coors,
                         const float *feats, int64_t m, int batch, int d, int h, int w, float *out8,
                         void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_pcr_loss_bwd_f32(const float *gen_offset, const float *gen_mask, const int32_t *coors,
                         const float *feats, int64_t m, int batch, int d, int h, int w,
                         const float *fwd_out8, const float *go_mask, const float *go_offset,
                         float *g_gen_mask, float *g_gen_offset_zeroed, s2d_stream_t stream);

/*
 * Layout + precision hand-over between the bf16 NHWC neck and the fp32 planar PCR head (rpn.py:283-285): tiled transposes,
 * x bf16 [batch][hw][c] <-> y fp32 [batch][c][hw].  c % 8 == 0, hw % 4 == 0.
 */
int s2d_nhwc_bf16_to_nchw_f32(const void *x, int batch, int c, int64_t hw, float *y, s2d_stream_t stream);
int s2d_nchw_f32_to_nhwc_bf16(const float *x, int batch, int c, int64_t hw, void *y, s2d_stream_t stream);
/* r05: the same hand-overs against NHWC rows of `ld` >= c channels (the first c are used; the writer zero-fills the rest): the PCR head's first
 * 1x1x1 conv (necks/rpn.py:263-266 `generator_1[0]` on `out_conv(F_S_b).view(n, 128, 5, h, w)`) runs as ONE 1x1 conv on the NHWC map with a
 * block-diagonal weight whose output channel count is padded to the tile kernels' multiple of 64 */
int s2d_nhwc_bf16_to_nchw_f32_ld(const void *x, int batch, int c, int ld, int64_t hw, float *y, s2d_stream_t stream);
int s2d_nchw_f32_to_nhwc_bf16_ld(const float *x, int batch, int c, int ld, int64_t hw, void *y, s2d_stream_t stream);

/* 2 x 2 resampling of NHWC bf16 maps (r04, the pillar S2D module): nn.Upsample(scale_factor=2, mode="nearest") and nn.MaxPool2d(2, 2) with
 * their backward passes; c % 8 == 0.  The max-pool backward re-derives the selected window element from x (torch's scan order, NaN
 * propagating) - no index tensor. */
int s2d_upsample2x_nhwc_bf16(const void *x, int n, int h, int w, int c, void *y, s2d_stream_t stream);
int s2d_upsample2x_bwd_nhwc_bf16(const void *dy, int n, int h, int w, int c, void *dx, s2d_stream_t stream);
/* 2 x 2 space-to-depth on NHWC bf16 (r06): x[n][2h][2w][c] -> y[n][h][w][(py, px, c)] (to_depth != 0), or its inverse (to_depth == 0: x is the
 * depth image, y the space image); h, w = the extent of the depth image, c % 8 == 0.  The rearrangements around nn.Conv2d(kernel 2, stride 2)
 * and nn.ConvTranspose2d(kernel 2, stride 2) when those run as 1x1 tile kernels (/root/reference/det3d/models/necks/rpn.py:188 and :92-104;
 * replaces torch's permute + contiguous copies there). */
int s2d_space_depth2_nhwc_bf16(const void *x, int n, int h, int w, int c, int to_depth, void *y, s2d_stream_t stream);
int s2d_maxpool2x2_nhwc_bf16(const void *x, int n, int h, int w, int c, void *y, s2d_stream_t stream);
int s2d_maxpool2x2_bwd_nhwc_bf16(const void *x, const void *dy, int n, int h, int w, int c, void *dx, s2d_stream_t stream);

/*
 * LayerNorm over a whole [C,H,W] map per sample (nn.LayerNorm([256,47,47]) of the S2D ConvNeXt blocks, det3d/models/necks/rpn.py:
 * 210-247): each row is split over many workgroups (two-level fixed-order reduction).  x / y / dy / dx: bf16 [batch][row] in
 * MEMORY order; weight / bias and their gradients: fp32 [row] in that same order (the caller permutes); row % 8 == 0;
 * stats [batch][2] = (mean, rstd).  bwd: dx, dweight, dbias are each optional.
 */
size_t s2d_lnwide_workspace_bytes(int batch);
int s2d_lnwide_fwd_bf16(const void *x, const float *weight, const float *bias, int batch, int64_t row, float eps,
                        void *y, float *stats, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_lnwide_bwd_bf16(const void *dy, const void *x, const float *weight, const float *stats, int batch,
                        int64_t row, void *dx, float *dweight, float *dbias, void *ws, size_t ws_bytes,
                        s2d_stream_t stream);

/* CenterHead losses on the device maps (csrc/center_loss.hip), one pass per direction; they replace the torch-op chains of
 * FastFocalLoss / RegLoss (/root/reference/det3d/models/losses/centernet_loss.py:33-54 and :9-31; call site
 * /root/reference/det3d/models/bbox_heads/center_head.py:236-283).  out / target / feat: fp32 [batch][c][hw] contiguous; ind, cat: int64
 * [batch][max_objs]; mask: uint8 [batch][max_objs]; reg target: fp32 [batch][max_objs][channels].
 * focal res (device, 4 floats): loss = -(pos + neg) / max(num_pos, 1), pos, neg, num_pos.  regloss res (device, channels + 1 floats):
 * loss per channel, then sum(mask) + 1e-4.  The backward entries scale by the device scalar(s) `go`. */
size_t s2d_focal_workspace_bytes(void);
int s2d_focal_fwd(const float *out, const float *target, const int64_t *ind, const uint8_t *mask, const int64_t *cat, int batch, int classes,
                  int64_t hw, int max_objs, float *res, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_focal_bwd(const float *out, const float *target, const int64_t *ind, const uint8_t *mask, const int64_t *cat, int batch, int classes,
                  int64_t hw, int max_objs, const float *res, const float *go, float *dout, s2d_stream_t stream);
int s2d_regloss_fwd(const float *feat, const int64_t *ind, const uint8_t *mask, const float *target, int batch, int channels, int64_t hw,
                    int max_objs, float *res, s2d_stream_t stream);
int s2d_regloss_bwd(const float *feat, const int64_t *ind, const uint8_t *mask, const float *target, int batch, int channels, int64_t hw,
                    int max_objs, const float *res, const float *go, float *dfeat, s2d_stream_t stream);

/*
 * The two losses for ALL tasks of a CenterHead in one node (the six-task nuScenes head): from the heat-map LOGITS and the branch maps
 * as the head produced them.  One record per task, passed as a HOST array (it travels in the kernel arguments); every map fp32
 * contiguous [batch][channels][hw]: hm_logit / hm (target) / p [classes], reg [2], height [1], dim [3], vel [2] (NULL for every task
 * of a head without a velocity branch: the target columns are then [0..5, 8, 9]), rot [2]; ind, cat int64 and mask uint8
 * [batch][max_objs]; anno_box fp32 [batch][max_objs][10].  fwd writes p = clamp(sigmoid(hm_logit), 1e-4, 1 - 1e-4), loss / loc_loss
 * [num_tasks] and res [num_tasks][16] = loss, hm_loss, loc_loss, loc_loss_elem[10], num_positive, 0, 0 with
 * loss = hm_loss + weight * sum_c code_weights[c] * loc_loss_elem[c] (code_weights: device, 10 floats with vel, else 8).  Same inputs,
 * same bits.  bwd writes d_logit of every task in full and scatters into d_reg .. d_rot, which must lie inside [dbranch, dbranch +
 * dbranch_bytes) - zero-filled by the entry; go_loss / go_loc: device [num_tasks] upstream gradients of loss / loc_loss (NULL = zero).
 */
typedef struct s2d_center_task {
    const float *hm_logit, *reg, *height, *dim, *vel, *rot;
    const float *hm;
    const int64_t *ind;
    const uint8_t *mask;
    const int64_t *cat;
    const float *anno_box;
    float *p;
    float *d_logit, *d_reg, *d_height, *d_dim, *d_vel, *d_rot;   /* bwd only */
    int classes;
} s2d_center_task;
size_t s2d_center_tasks_loss_workspace_bytes(void);
int s2d_center_tasks_loss_fwd(const s2d_center_task *tasks, int num_tasks, int batch, int64_t hw, int max_objs,
                              const float *code_weights, float weight, float *loss, float *loc_loss, float *res, void *ws,
                              size_t ws_bytes, s2d_stream_t stream);
int s2d_center_tasks_loss_bwd(const s2d_center_task *tasks, int num_tasks, int batch, int64_t hw, int max_objs,
                              const float *code_weights, float weight, const float *res, const float *go_loss,
                              const float *go_loc, void *dbranch, size_t dbranch_bytes, s2d_stream_t stream);

/*
 * Feature-distillation loss of the S2D step (det3d/torchie/trainer/trainer.py:783-789): w_pos * MSE over teacher > 0 + w_neg * MSE
 * over the rest, between two dense tensors of n elements (n % 8 == 0) in the SAME memory order, bf16 (flag 1) or fp32 (0) each.
 * out4 (device) = loss, 2*w_pos/n_pos, 2*w_neg/n_neg, n_pos.  bwd: dstudent (student's element type) = go * dloss/dstudent.
 */
size_t s2d_masked_mse_workspace_bytes(void);
int s2d_masked_mse_fwd(const void *student, int student_bf16, const void *teacher, int teacher_bf16, int64_t n, float w_pos,
                       float w_neg, float *out4, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_masked_mse_bwd(const void *student, int student_bf16, const void *teacher, int teacher_bf16, int64_t n,
                       const float *fwd_out4, const float *go, void *dstudent, s2d_stream_t stream);

/*
 * Feature loss of the PointPillars distillation branch (det3d/torchie/trainer/trainer.py:749-762): the four maps [n, c, h, w] are
 * max-pooled 2x2 (floor mode) on the fly and five masked MSE terms of weight 10 are taken over the pooled values, the masks being
 * pooled teacher > 0; the third term puts the `a` maps under the `b` mask.  sa, sb: the student's maps, one element type
 * (student_bf16: 1 bf16, 0 fp32) and one memory order (student_nhwc: 1 channels_last, 0 planar); da, db: the teacher's, likewise.
 * c % 8 == 0, h >= 2, w >= 2, 16-byte aligned maps; anything else is S2D_ERR_UNSUPPORTED.
 * out8 (device) = loss, 20/nA, 20/(N-nA), 20/nB, 20/nB, 20/(N-nB), nA, nB.  Deterministic (no atomics), no host read, no memset.
 * bwd: dsa, dsb (the student's element type and order) = go * dloss/dstudent, routed to each window's selected element by torch's
 * max_pool2d rule (first of tied elements); every element is written once, zeros included.
 */
size_t s2d_pooled_distill_workspace_bytes(void);
int s2d_pooled_distill_fwd(const void *sa, const void *sb, int student_bf16, int student_nhwc, const void *da, const void *db,
                           int teacher_bf16, int teacher_nhwc, int n, int c, int h, int w, float *out8, void *ws, size_t ws_bytes,
                           s2d_stream_t stream);
int s2d_pooled_distill_bwd(const void *sa, const void *sb, int student_bf16, int student_nhwc, const void *da, const void *db,
                           int teacher_bf16, int teacher_nhwc, int n, int c, int h, int w, const float *out8, const float *go,
                           void *dsa, void *dsb, s2d_stream_t stream);

/*
 * Fused PCR level heads + losses: gen_mask_k / gen_out_k (1x1x1 Conv3d C->1 / C->3, det3d/models/necks/rpn.py:273-275,292-294)
 * and mask_offset_loss (voxelnet.py:171-185) evaluated straight from the level's feature volume g[B][C][D*H*W] - the occupancy
 * logits, the offset volume and its zero-filled gradient are never written; the offset conv runs at the m recon voxels only.
 * head_params (device, 4C+4 floats) = w_mask[C] | w_off[3][C] | b_mask | b_off[3].  out8 as s2d_pcr_loss_fwd_f32.
 * bwd writes dg[B][C][cells] = w_mask*dL/dlogit (+ w2^T.dz when co > 0: the data gradient of the level's next 1x1x1 conv
 * g -> z[B][co][cells], w2[co][C]) plus the sparse corrections, and dw_mask[C], db_mask[1], dw_off[3][C], db_off[3].
 * Supported: (C, co) in {(32,0), (32,16), (3,0)}, cells % 4 == 0.
 */
int s2d_pcr_heads_supported(int c, int co, int64_t cells);
size_t s2d_pcr_heads_workspace_bytes(int c);
int s2d_pcr_heads_fwd_f32(const float *g, const float *head_params, const int32_t *coors, const float *feats,
                          int64_t m, int batch, int c, int d, int h, int w, float *out8, void *ws,
                          size_t ws_bytes, s2d_stream_t stream);
int s2d_pcr_heads_bwd_f32(const float *g, const float *head_params, const int32_t *coors, const float *feats,
                          int64_t m, int batch, int c, int d, int h, int w, const float *fwd_out8,
                          const float *go_mask, const float *go_offset, const float *dz, const float *w2, int co,
                          float *dg, float *dw_mask, float *db_mask, float *dw_off, float *db_off, void *ws,
                          size_t ws_bytes, s2d_stream_t stream);

/*
 * The same level with the preceding BatchNorm3d + ReLU folded in (rpn.py:265-272,287-291): y is the RAW ConvTranspose3d output,
 * g = relu(y*scale + shift) is applied on the fly (bn_scale_shift, device, 2C = scale[C] | shift[C]); neither g, its gradient nor
 * the masked batch-norm gradient is written.  fwd also writes z[B][co][cells] = w2.g + b2 when co > 0.  The backward is two
 * passes around the batch norm's own finalisation: bwd_sums -> grads[4C+4] = dw_mask | dw_off | db_mask | db_off and bn_sums[2C] =
 * (sum dG*m, sum dG*m*y) (what s2d_bncm_bwd_reduce_f32 produces); bwd_apply -> dy = a*dG*m + b*y + d with abd (device, 3C).
 */
size_t s2d_pcr_level_workspace_bytes(int c);
int s2d_pcr_level_fwd_f32(const float *y, const float *bn_scale_shift, const float *head_params, const float *w2,
                          const float *b2, const int32_t *coors, const float *feats, int64_t m, int batch, int c,
                          int co, int d, int h, int w, float *z, float *z_stats /* [2 co] sum | sumsq of z per channel (the
                          statistics of the BatchNorm3d behind the 1x1x1 conv; c = 32, co = 16 only), or NULL */, float *out8,
                          void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_pcr_level_bwd_sums_f32(const float *y, const float *bn_scale_shift, const float *head_params,
                               const int32_t *coors, const float *feats, int64_t m, int batch, int c, int d, int h,
                               int w, const float *fwd_out8, const float *go_mask, const float *go_offset,
                               const float *dz, const float *w2, int co, float *grads, float *bn_sums, void *ws,
                               size_t ws_bytes, s2d_stream_t stream);
int s2d_pcr_level_bwd_apply_f32(const float *y, const float *bn_scale_shift, const float *head_params,
                                const int32_t *coors, const float *feats, int64_t m, int batch, int c, int d, int h,
                                int w, const float *fwd_out8, const float *go_mask, const float *go_offset,
                                const float *dz, const float *w2, int co, const float *abd, float *dy,
                                s2d_stream_t stream);

/*
 * Rotated bird's-eye-view IoU and greedy NMS of CenterHead.predict (det3d/core/bbox/box_torch_ops.py:449-464 rotate_nms_pcdet,
 * det3d/ops/iou3d_nms/src/iou3d_nms_kernel.cu:236-326, src/iou3d_nms.cpp:92-130).  Boxes: 7 floats (x,y,z,dx,dy,dz,heading).
 * s2d_nms_rotated_bev takes the boxes SORTED by descending score and writes the kept indices (into that order) and their count
 * to device memory - the suppression matrix is walked on the device, no host round trip.
 */
int s2d_bev_iou_f32(const float *boxes_a, int na, const float *boxes_b, int nb, float *iou, s2d_stream_t stream);
size_t s2d_nms_workspace_bytes(int n);
int s2d_nms_rotated_bev(const float *boxes_sorted, int n, float iou_threshold, int max_keep, int64_t *keep,
                        int32_t *n_keep, void *ws, size_t ws_bytes, s2d_stream_t stream);
/* CenterPoint's circle NMS (det3d/core/utils/circle_nms_jit.py:4-31, called from bbox_heads/center_head.py:476-479,499-507): greedy
 * suppression by centre distance - a later box is removed when (xi - xj)^2 + (yi - yj)^2 <= thresh (the reference compares the squared
 * distance with test_cfg.min_radius[task] as is).  xy_sorted: [n][2] centres sorted by descending score; same outputs and workspace
 * (s2d_nms_workspace_bytes) as s2d_nms_rotated_bev. */
int s2d_nms_circle(const float *xy_sorted, int n, float thresh, int max_keep, int64_t *keep, int32_t *n_keep, void *ws, size_t ws_bytes,
                   s2d_stream_t stream);

/*
 * CenterHead.predict on the device for ALL tasks and samples of a head at once (csrc/center_predict.hip).  A SEGMENT is one
 * (task, sample) pair, segment = task * samples + sample.  One record per task, passed as a HOST array of 1..8 entries (it travels in
 * the kernel arguments): the fp32 maps hm [classes], reg [2], height [1], dim [3], vel [2] (NULL for every task of a head without a
 * velocity branch: boxes then have 7 floats, else 9), rot [2], each [images][channels][h][w] with images = samples (4 * samples with
 * double_flip: every sample as original, H-mirrored, W-mirrored, both), image stride channels * h * w, and element (c, pixel) at
 * c * channel_stride + pixel * pixel_stride - NCHW-contiguous (h * w, 1) and channels_last (1, channels) maps are read in place.
 *
 * s2d_center_predict_score replaces det3d/models/bbox_heads/center_head.py:311-362,384-401 (permute, flips, sigmoid, the means, the
 * centre) and :459-465 (maximum over classes, score and centre-range masks): score [segments][h * w] = the class maximum of
 * mean(sigmoid(hm)) or -inf where `score > score_threshold` is false (NaN included) or the centre (x, y, z) lies outside range6 (HOST,
 * xmin ymin zmin xmax ymax zmax, inclusive; NULL = no test); label [segments][h * w] = its class (lowest index on a tie); count
 * [segments] = passing pixels.  x = (col + reg_x) * out_size_factor * voxel_x + pc_x, y likewise from the row.
 *
 * s2d_center_predict_boxes replaces center_head.py:344,364-382,403-419 (exp, rotation and velocity sign rules, atan2, cat) and the
 * mask / sort gathers of :467-471,483-485 for the candidates only: with order / score_sorted [segments][h * w] the descending stable
 * sort of `score` along its last axis, rank r < min(counts[s], max_count) of segment s becomes row offsets[s] + r of the packed
 * lists boxes [total][7 or 9] = x, y, z, mean(exp(dim)), (vel,) atan2(rot_sin, rot_cos); scores [total]; labels [total] (int64, class +
 * label_base of the task).  offsets / counts: DEVICE int32 [segments]; rows outside [0, total) are not written.
 */
#define S2D_CENTER_PREDICT_MAX_TASKS 8
typedef struct s2d_center_predict_task {
    const float *map[6];   /* hm, reg, height, dim, vel, rot */
    int64_t channel_stride[6], pixel_stride[6];
    int classes;
    int label_base;
} s2d_center_predict_task;
int s2d_center_predict_score(const s2d_center_predict_task *tasks, int num_tasks, int samples, int h, int w, int double_flip,
                             float score_threshold, const float *range6, float out_size_factor, float voxel_x, float voxel_y, float pc_x,
                             float pc_y, float *score, int32_t *label, int32_t *count, s2d_stream_t stream);
int s2d_center_predict_boxes(const s2d_center_predict_task *tasks, int num_tasks, int samples, int h, int w, int double_flip,
                             float out_size_factor, float voxel_x, float voxel_y, float pc_x, float pc_y, const int64_t *order,
                             const float *score_sorted, const int32_t *label, const int32_t *offsets, const int32_t *counts, int max_count,
                             int64_t total, float *boxes, float *scores, int64_t *labels, s2d_stream_t stream);

/*
 * The two greedy NMS forms above for MANY independent segments in two launches; replaces the per-(task, sample) loop of
 * center_head.py:455-481 over box_torch_ops.py:449-464 (rotate_nms_pcdet) / center_head.py:499-507 (_circle_nms): one kernel fills the
 * suppression bits of every segment, one walks them with a workgroup per segment.  Segment s = rows offsets[s] .. offsets[s] +
 * min(counts[s], max_count) of a packed list of `total` rows sorted by descending score inside each segment (DEVICE int32 arrays;
 * max_count <= 65536; a segment reaching outside [0, total) counts as empty).  Rotated form: rows of box_stride >= 7 floats, x y z dx dy
 * dz first and the heading LAST (7- and 9-float boxes alike).  Circle form: (x, y) first in rows of xy_stride floats, thresh DEVICE
 * [segments] (test_cfg.min_radius of the segment's task, compared with the squared distance as the reference does).
 * Outputs: keep [segments][max_keep] int64 indices into the segment's own rows, n_keep [segments] - written for EVERY segment, empty
 * ones included; keep entries past n_keep[s] are left untouched.  Workspace: s2d_nms_batched_workspace_bytes(total, max_count).
 */
size_t s2d_nms_batched_workspace_bytes(int64_t total, int max_count);
int s2d_nms_rotated_bev_batched(const float *boxes, int box_stride, const int32_t *offsets, const int32_t *counts, int segments,
                                int max_count, int64_t total, float iou_threshold, int max_keep, int64_t *keep, int32_t *n_keep, void *ws,
                                size_t ws_bytes, s2d_stream_t stream);
int s2d_nms_circle_batched(const float *xy, int xy_stride, const int32_t *offsets, const int32_t *counts, int segments, int max_count,
                           int64_t total, const float *thresh, int max_keep, int64_t *keep, int32_t *n_keep, void *ws, size_t ws_bytes,
                           s2d_stream_t stream);

/*
 * The two kernels that let CenterHead.predict run without the host (center_predict.StaticPredictPlan): a selection in place of the full
 * sort of the score rows, and an assembly into outputs of fixed capacity.
 *
 * s2d_segment_topk (csrc/segment_topk.hip), one workgroup per row, no communication between workgroups: for every row s of score
 * [segments][row_stride] (row_len <= row_stride, row_len <= 2^20, 1 <= k <= 4096) ranks r < min(k, row_len) of the row's STABLE
 * DESCENDING sort go to order[s * out_stride + r] (int64 index into the row) and score_sorted[s * out_stride + r] (the element, bit for
 * bit); entries at r >= min(k, row_len) are not touched.  Comparison is by float value: -0.0 == +0.0, -inf is the lowest value, equal
 * values go in ascending index order - the first k columns of torch.sort(row, descending=True, stable=True).  NaN is outside the
 * contract (the score kernel never writes it); it costs no out-of-bounds access.  With passed (DEVICE int32 [segments], the pass counts
 * s2d_center_predict_score wrote) the entry also writes the segment table of the packed lists of k rows per segment that
 * s2d_center_predict_boxes and the batched NMS read: offsets[s] = s * k, counts[s] = min(passed[s], k), overflow[s] = passed[s] > k
 * (all DEVICE int32 [segments]); passed == NULL: no table.
 *
 * s2d_predict_static_gather (csrc/center_predict.hip), one workgroup per sample: walks the sample's tasks in task order and copies the
 * first min(n_keep[s], max_keep) kept rows keep[s][i] (indices into the segment's own rows, from row offsets[s] of the packed lists of
 * `total` rows) of each segment s = task * samples + sample into boxes [samples][cap][box_dim], scores [samples][cap], labels
 * [samples][cap] (int64), cap = tasks * max_keep, and their number into counts [samples] (int32).  Rows at or past counts[b] are written
 * too: boxes and scores zero, label -1.
 */
int s2d_segment_topk(const float *score, int segments, int64_t row_len, int64_t row_stride, int k, const int32_t *passed, int64_t *order,
                     float *score_sorted, int64_t out_stride, int32_t *offsets, int32_t *counts, int32_t *overflow, s2d_stream_t stream);
int s2d_predict_static_gather(const float *cand_boxes, const float *cand_scores, const int64_t *cand_labels, const int32_t *offsets,
                              const int64_t *keep, const int32_t *n_keep, int tasks, int samples, int max_keep, int box_dim, int64_t total,
                              float *boxes, float *scores, int64_t *labels, int32_t *counts, s2d_stream_t stream);

/*
 * CenterPoint training targets on the device = AssignLabel.__call__ (det3d/datasets/pipelines/preprocess.py:489-653, one-task
 * Waymo head) with gaussian_radius / draw_umich_gaussian (det3d/core/utils/center_utils.py:18-64).  gt_boxes fp32
 * [frames][max_boxes][9] (x,y,z,w,l,h,vx,vy,yaw), gt_classes int32 [frames][max_boxes] (1-based, <= 0 = padding).  Outputs per
 * frame: hm fp32 [num_classes][fmap_h][fmap_w] (ZEROED by the caller), anno_box fp32 [max_objs][10], ind int64 [max_objs],
 * mask uint8 [max_objs], cat int64 [max_objs], gt_boxes_and_cls fp32 [max_objs][10] (optional, two-stage code).
 */
int s2d_assign_label(const float *gt_boxes, const int32_t *gt_classes, int frames, int max_boxes,
                     const float pc_range_xy[2], const float voxel_size_xy[2], int out_size_factor, int fmap_w,
                     int fmap_h, int num_classes, int max_objs, double gaussian_overlap, int min_radius,
                     float *hm_zeroed, float *anno_box, int64_t *ind, uint8_t *mask, int64_t *cat,
                     float *gt_boxes_and_cls, s2d_stream_t stream);
/*
 * The same for a table of tasks (AssignLabel with the six-task nuScenes table), from boxes in the frame's ORIGINAL order: gt_classes are
 * the global 1-based classes (<= 0 or above the last class of the table: ignored), task_num_classes a HOST array of num_tasks (<= 8)
 * class counts; task t owns the classes off_t+1 .. off_t+n_t.  Slot k of a task is its k-th object in (class, original index) order,
 * objects with k >= max_objs are dropped.  Outputs are laid out task after task: hm fp32 [frames][n_t][fmap_h][fmap_w] per task at plane
 * offset frames * off_t (ZEROED by the caller), anno_box fp32 [tasks][frames][max_objs][10], ind int64 / mask uint8 / cat int64 (class
 * inside the task) [tasks][frames][max_objs] - all fully written - and, optional, gt_boxes_and_cls fp32 [frames][max_objs][10] =
 * (x,y,z,w,l,h,yaw,vx,vy,global class) over the flattened task order, cut at max_objs rows (the reference asserts that they fit).
 */
int s2d_assign_label_tasks(const float *gt_boxes, const int32_t *gt_classes, int frames, int max_boxes,
                           const int32_t *task_num_classes, int num_tasks, const float pc_range_xy[2],
                           const float voxel_size_xy[2], int out_size_factor, int fmap_w, int fmap_h, int max_objs,
                           double gaussian_overlap, int min_radius, float *hm_zeroed, float *anno_box, int64_t *ind,
                           uint8_t *mask, int64_t *cat, float *gt_boxes_and_cls, s2d_stream_t stream);

/*
 * SECOND anchor head (csrc/anchor_head.hip), Waymo configuration: ground_box3d_coder 7-wide (x,y,z,w,l,h,r), nearest-IoU similarity, no
 * sampling, no anchors_mask.  anchors: fp32 [num_anchors][7], shared by the frames; anchor a sits in slot a % (num_classes * rotations) of
 * its cell and slots [c * rotations, (c + 1) * rotations) belong to class c (det3d/core/anchor/target_assigner.py:139-158).
 *
 * s2d_anchor_assign = AssignTarget.__call__ in train mode (det3d/datasets/pipelines/preprocess.py:726-830: per-class split,
 * limit_period(yaw, 0.5, 2 pi)) over TargetAssigner.assign_v2 (target_assigner.py:68-137) and create_target_np
 * (det3d/core/anchor/target_ops.py:29-223) with rbbox2d_to_near_bbox / iou_jit(eps = 0) / second_box_encode
 * (det3d/core/bbox/box_np_ops.py:131-143,497-535,1002-1063).  gt_boxes fp32 [frames][max_boxes][7], gt_classes int32 [frames][max_boxes]
 * (1-based; <= 0 = padding; max_boxes <= 500); matched / unmatched thresholds: HOST arrays of num_classes floats.  Outputs: labels int32
 * [frames][num_anchors] (-1 ignore, 0 negative, class id positive), reg_targets fp32 [frames][num_anchors][7], reg_weights fp32
 * [frames][num_anchors].  Overlaps are computed with float64 intermediates and rounded once to fp32, as the numba loop does.
 */
size_t s2d_anchor_assign_workspace_bytes(int frames, int max_boxes);
int s2d_anchor_assign(const float *gt_boxes, const int32_t *gt_classes, int frames, int max_boxes, const float *anchors,
                      int64_t num_anchors, int num_classes, int rotations, const float *matched_thresholds,
                      const float *unmatched_thresholds, int32_t *labels, float *reg_targets, float *reg_weights, void *ws,
                      size_t ws_bytes, s2d_stream_t stream);
/*
 * MultiGroupHead.loss for one task (det3d/models/bbox_heads/mg_head.py:535-667 with prepare_loss_weights NormByNumPositives, create_loss,
 * add_sin_difference, get_direction_target, _get_pos_neg_loss of mg_head.py:29-63,147-188 and SigmoidFocalLoss / WeightedSmoothL1Loss
 * (codewise) / WeightedSoftmaxClassificationLoss of det3d/models/losses/losses.py:147-222,293-359,431-469).  box_preds fp32
 * [frames][num_anchors][7], cls_preds [frames][num_anchors][num_classes], dir_cls_preds [frames][num_anchors][2] (the NHWC head outputs).
 * params: HOST array of 9 floats - pos_cls_weight, neg_cls_weight, focal alpha, focal gamma (must be 2), smooth-L1 sigma, loss weights of
 * loc / cls / dir, direction_offset.  res (device, 15 floats): loss, cls_pos_loss, cls_neg_loss, dir_loss_reduced, cls_loss_reduced,
 * loc_loss_reduced, loc_loss_elem[7], num_pos and num_neg of frame 0.  norm (device, frames floats): 1 / clamp(positives of the frame, 1),
 * read by the backward.  _bwd: d_* = grad_loss[0] (device scalar) * d loss / d preds, every element written.
 */
size_t s2d_anchor_loss_workspace_bytes(int frames);
int s2d_anchor_loss_fwd(const float *box_preds, const float *cls_preds, const float *dir_cls_preds, const int32_t *labels,
                        const float *reg_targets, const float *anchors, int frames, int64_t num_anchors, int num_classes,
                        const float *params, float *res, float *norm, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_anchor_loss_bwd(const float *box_preds, const float *cls_preds, const float *dir_cls_preds, const int32_t *labels,
                        const float *reg_targets, const float *anchors, int frames, int64_t num_anchors, int num_classes,
                        const float *params, const float *norm, const float *grad_loss, float *d_box_preds, float *d_cls_preds,
                        float *d_dir_cls_preds, s2d_stream_t stream);
/*
 * The per-anchor part of MultiGroupHead.predict (mg_head.py:737-765,838-849,995-1001): second_box_decode
 * (det3d/core/bbox/box_torch_ops.py:87-150) -> boxes fp32 [frames][num_anchors][7]; scores = max sigmoid(cls) and its class -> labels
 * int32; dir_labels = argmax(dir_cls_preds) (0 when dir_cls_preds is null); keep uint8 = scores >= score_threshold.
 */
int s2d_anchor_decode(const float *box_preds, const float *cls_preds, const float *dir_cls_preds, const float *anchors, int frames,
                      int64_t num_anchors, int num_classes, float score_threshold, float *boxes, float *scores, int32_t *labels,
                      int32_t *dir_labels, uint8_t *keep, s2d_stream_t stream);

/*
 * MultiGroupHead.predict on the device for ALL tasks and samples of a head at once (csrc/anchor_predict.hip; mg_head.py:697-1086,
 * single-class rotated-NMS branch).  A SEGMENT is one (task, sample) pair, segment = task * samples + sample.  One record per task, passed
 * as a HOST array of 1..8 entries (it travels in the kernel arguments): the contiguous fp32 head outputs box_preds [samples][num_anchors][7],
 * cls_preds [samples][num_anchors][classes], dir_cls_preds [samples][num_anchors][2] (NULL: no direction classifier, direction label 0) and
 * the anchor table [num_anchors][7].  max_anchors >= every task's num_anchors is the row length of the score maps.
 *
 * s2d_anchor_predict_score: score [segments][max_anchors] = the class maximum of sigmoid(cls_preds) (the expression of s2d_anchor_decode)
 * where it is >= score_threshold, else -1 (a NaN maximum and the columns past the task's num_anchors included); label
 * [segments][max_anchors] = its class (lowest index on a tie); count [segments] = passing anchors.
 *
 * s2d_anchor_predict_boxes: with order / score_sorted [segments][max_anchors] the descending stable sort of `score` along its last axis,
 * rank r < min(counts[s], max_count) of segment s becomes row offsets[s] + r of the packed lists: boxes [total][7] = second_box_decode
 * in the form the rotated NMS takes, (x, y, z, w, l, h, -r) (the arithmetic of s2d_anchor_decode, bit for bit); scores [total]; labels
 * [total] (class inside the task); dir_labels [total] = argmax(dir_cls_preds); in_range [total] = 1 when the centre (x, y, z) lies inside
 * range6 (HOST, xmin ymin zmin xmax ymax zmax, inclusive; NULL = every row is inside).  offsets / counts: DEVICE int32 [segments]; rows
 * outside [0, total) are not written.
 *
 * s2d_anchor_predict_finish: after s2d_nms_rotated_bev_batched on those rows (keep [segments][max_keep], n_keep [segments], both on the
 * DEVICE), one workgroup per segment walks the first min(n_keep[s], max_keep) kept rows in order, drops those whose in_range flag is
 * clear, and writes out_boxes [segments][max_keep][7] = (x, y, z, w, l, h, r) with r + pi (fp32 pi) where use_direction and
 * ((r - direction_offset) > 0) != (dir_label != 0) (mg_head.py:1057-1066), out_scores [segments][max_keep], out_labels
 * [segments][max_keep] (int64, class + the task's label_base; of the task records only label_base is read) and out_count [segments] -
 * written for EVERY segment; entries past out_count[s] are left untouched.
 *
 * s2d_anchor_predict_finish_static (the static path, anchor_predict.StaticAnchorPlan): the same finish with one workgroup per SAMPLE b.
 * It walks the sample's tasks in task order, every segment s = task * samples + b as above (the same per-row arithmetic, bit for bit; a
 * segment reaching outside [0, total) counts as empty), and writes the surviving rows contiguously from row 0 of out_boxes
 * [samples][cap][7], out_scores [samples][cap], out_labels [samples][cap] (int64), cap = num_tasks * max_keep, and their number into
 * out_counts [samples] (int32).  Rows at or past out_counts[b] are written at every call: boxes and scores zero, label -1.  No atomics,
 * no communication between workgroups.  Refused with S2D_ERR_ARG before any HIP call: a null pointer, num_tasks outside 1..8, a negative
 * size, num_tasks * samples > 65535; samples == 0 succeeds without a launch.
 */
#define S2D_ANCHOR_PREDICT_MAX_TASKS 8
typedef struct s2d_anchor_predict_task {
    const float *box_preds, *cls_preds, *dir_cls_preds, *anchors;
    int64_t num_anchors;
    int classes;
    int label_base;   /* added to the labels of the task by s2d_anchor_predict_finish */
} s2d_anchor_predict_task;
int s2d_anchor_predict_score(const s2d_anchor_predict_task *tasks, int num_tasks, int samples, int64_t max_anchors,
                             float score_threshold, float *score, int32_t *label, int32_t *count, s2d_stream_t stream);
int s2d_anchor_predict_boxes(const s2d_anchor_predict_task *tasks, int num_tasks, int samples, int64_t max_anchors,
                             const float *range6, const int64_t *order, const float *score_sorted, const int32_t *label,
                             const int32_t *offsets, const int32_t *counts, int max_count, int64_t total, float *boxes, float *scores,
                             int32_t *labels, int32_t *dir_labels, uint8_t *in_range, s2d_stream_t stream);
int s2d_anchor_predict_finish(const s2d_anchor_predict_task *tasks, int num_tasks, int samples, const float *boxes, const float *scores,
                              const int32_t *labels, const int32_t *dir_labels, const uint8_t *in_range, const int32_t *offsets,
                              const int32_t *counts, int64_t total, const int64_t *keep, const int32_t *n_keep, int max_keep,
                              int use_direction, float direction_offset, float *out_boxes, float *out_scores,
                              int64_t *out_labels, int32_t *out_count, s2d_stream_t stream);
int s2d_anchor_predict_finish_static(const s2d_anchor_predict_task *tasks, int num_tasks, int samples, const float *boxes,
                                     const float *scores, const int32_t *labels, const int32_t *dir_labels, const uint8_t *in_range,
                                     const int32_t *offsets, const int32_t *counts, int64_t total, const int64_t *keep,
                                     const int32_t *n_keep, int max_keep, int use_direction, float direction_offset, float *out_boxes,
                                     float *out_scores, int64_t *out_labels, int32_t *out_counts, s2d_stream_t stream);

/*
 * Optimizer step of the reference's training loop (det3d/torchie/apis/train.py:168-186, det3d/solver/fastai_optim.py:158-171,
 * hooks/optimizer.py:15-21): gradient L2 norm -> clip coefficient (device scalar, clip_grad_norm_ semantics) -> fused
 * multi-tensor Adam with decoupled weight decay: p *= 1 - lr*wd; Adam(betas, eps) on grad*clip_coef with bias correction of
 * step `step` (1-based).  Up to s2d_adam_max_tensors() tensors per call (host pointer tables of DEVICE pointers).
 */
int s2d_adam_max_tensors(void);
int s2d_adam_step_f32(int count, float *const *params, const float *const *grads, float *const *exp_avg,
                      float *const *exp_avg_sq, const int64_t *numel, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int step, const float *clip_coef, s2d_stream_t stream);
size_t s2d_grad_norm_workspace_floats(int count, const int64_t *numel);
int s2d_grad_sumsq_f32(int count, const float *const *grads, const int64_t *numel, float *partial,
                       int *written, s2d_stream_t stream);
int s2d_grad_norm_finalize_f32(const float *partial, int n, float max_norm, float *out2, s2d_stream_t stream);

/*
 * SyncBN statistics all-reduce on the compute stream (det3d/torchie/apis/train.py:281-300: apex SyncBatchNorm + DDP when
 * training distributed).  The RCCL already loaded in the process is resolved at run time; s2d_comm_available() == 0 means
 * the host keeps using its own collective.  Bootstrap: rank 0 calls s2d_comm_unique_id (128 bytes), the host broadcasts
 * them, every rank calls s2d_comm_init (collective).  s2d_comm_allreduce_sum_f32: in-place sum of `count` floats over the
 * ranks, enqueued on `stream` (between a batch-norm reduction kernel and its finalize kernel).
 */
int s2d_comm_load_library(const char *path); /* optional: the RCCL shared object the host framework has loaded */
int s2d_comm_available(void);
int s2d_comm_unique_id(void *id128);
int s2d_comm_init(const void *id128, int nranks, int rank);
int s2d_comm_ranks(void);
int s2d_comm_shutdown(void);
int s2d_comm_allreduce_sum_f32(float *buf, int64_t count, s2d_stream_t stream);

/* r04: the weight images of up to 64 dense conv layers in ONE launch (the re-pack after an optimizer step; the reference has no such
 * step - its cuDNN/MIOpen convs read the fp32 parameters directly).  Per layer the arguments of s2d_conv2d{3x3,1x1}_pack_weights[_pair]_bf16;
 * packed_dgrad[i] = NULL packs a single image (with transpose_flip[i]).  Host arrays of device pointers / ints. */
int s2d_conv2d_pack_batch_bf16(int n, const float *const *weights, const int32_t *cin, const int32_t *cout, const int32_t *taps,
                               const int32_t *weight_nhwc, const int32_t *transpose_flip, void *const *packed_fwd, void *const *packed_dgrad,
                               s2d_stream_t stream);

/* ---- r04: bf16 storage of the raw PCR up-sampler outputs ---------------------------------------------------------------------
 * (det3d/models/necks/rpn.py:263-296: the outputs of the two ConvTranspose3d layers, 724 MB and 543 MB in fp32 at batch 4, are read by
 * four passes of the fused level each).  Same contracts as the fp32 entries named alike; only the element type of that tensor changes:
 * `out_bf16` / `y` / `in_bf16` are bf16 [B][C][cells]; every other tensor, the statistics and all accumulation stay fp32. */
int s2d_convt3d_mfma_fwd_stats_y16(const float *in, const void *packed, const float *bias, int batch, int cin, int cout, int d, int h, int w,
                                   void *out_bf16, float *stats_partial, s2d_stream_t stream);
int s2d_pointwise_conv_wgrad_norm_x16(const void *in_bf16, const float *in_scale_shift, const float *dout, int batch, int cin, int cout,
                                      int64_t positions, float *dweight, float *dbias, void *ws, size_t ws_bytes, s2d_stream_t stream);
/* r06: the 16-channel volume z between the two PCR levels ([B,16,10,376,376] at the benchmark: 362 MB in fp32), its gradient dz and the second
 * up-sampler's input gradient dx' STORED IN BF16 (fp32 arithmetic, sums and statistics everywhere): the twelve passes per step that cross one
 * of the three move half the bytes.  Same contracts as the entries they extend (rpn.py:263-296; replaces the same torch calls):
 *   s2d_pcr_level_fwd_y16_z16            = s2d_pcr_level_fwd_y16 writing z as bf16 (c = 32, co = 16; z_stats of the stored values)
 *   s2d_pcr_level_bwd_sums_y16_z16, s2d_pcr_level_bwd_apply_y16_d16_z16 = the level's backward passes reading a bf16 dz
 *   s2d_pointwise_conv_wgrad_norm_x16_d16 = s2d_pointwise_conv_wgrad_norm_x16 with a bf16 dout (cin = 32)
 *   s2d_convt3d_mfma_fwd_stats_y16_norm_x16, _wgrad_d16_norm_x16 = the up-sampler's forward / weight gradient reading a bf16 raw input
 *   s2d_convt3d_mfma_dgrad_d16_x16       = its data gradient written as bf16        (all three: s2d_convt3d_mfma_x16_supported shapes)
 *   s2d_bncm_bwd_reduce_x_typed / s2d_bncm_bwd_apply_x_typed = s2d_bncm_bwd_reduce_x_f32 / _apply_x_f32 with a storage flag per tensor
 *     (0 fp32, 1 bf16); combinations (x, dy, dx): all fp32 | (fp32, bf16, fp32) | all bf16 */
/* r06: per-voxel cache for the NEXT s2d_pcr_level_* call on the calling thread (any storage variant): the forward call fills row i with the c raw
 * values of y at recon voxel i's cell ([m][c] elements of y's type, [m][4] for c = 3), the level's two backward calls read their voxels from it
 * instead of c scattered loads per voxel.  buf: >= m * (c == 3 ? 4 : c) * sizeof(y element) bytes of device memory (smaller: ignored); consumed by
 * the next call, repeat per call; NULL / 0 clears.  (voxelnet.py:171-185: the per-voxel terms of the mask / offset losses.) */
int s2d_pcr_level_site_cache(void *buf, size_t bytes);
int s2d_pcr_level_fwd_y16_z16(const void *y, const float *bn_scale_shift, const float *head_params, const float *w2, const float *b2,
                              const int32_t *coors, const float *feats, int64_t m, int batch, int c, int co, int d, int h, int w, void *z_bf16,
                              float *z_stats, float *out8, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_pcr_level_bwd_sums_y16_z16(const void *y, const float *bn_scale_shift, const float *head_params, const int32_t *coors, const float *feats,
                                   int64_t m, int batch, int c, int d, int h, int w, const float *fwd_out8, const float *go_mask,
                                   const float *go_offset, const void *dz_bf16, const float *w2, int co, float *grads, float *bn_sums, void *ws,
                                   size_t ws_bytes, s2d_stream_t stream);
int s2d_pcr_level_bwd_apply_y16_d16_z16(const void *y, const float *bn_scale_shift, const float *head_params, const int32_t *coors,
                                        const float *feats, int64_t m, int batch, int c, int d, int h, int w, const float *fwd_out8,
                                        const float *go_mask, const float *go_offset, const void *dz_bf16, const float *w2, int co,
                                        const float *abd, void *dy_bf16, s2d_stream_t stream);
int s2d_pointwise_conv_wgrad_norm_x16_d16(const void *in_bf16, const float *in_scale_shift, const void *dout_bf16, int batch, int cin, int cout,
                                          int64_t positions, float *dweight, float *dbias, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_convt3d_mfma_x16_supported(int cin, int cout, int d, int h, int w);
int s2d_convt3d_mfma_fwd_stats_y16_norm_x16(const void *in_bf16, const float *in_scale_shift, const void *packed, const float *bias, int batch,
                                            int cin, int cout, int d, int h, int w, void *out_bf16, float *stats_partial, s2d_stream_t stream);
int s2d_convt3d_mfma_wgrad_d16_norm_x16(const void *in_bf16, const float *in_scale_shift, const void *dout_bf16, int batch, int cin, int cout,
                                        int d, int h, int w, float *dweight, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_convt3d_mfma_dgrad_d16_x16(const void *dout_bf16, const void *packed, int batch, int cin, int cout, int d, int h, int w, void *din_bf16,
                                   s2d_stream_t stream);
int s2d_bncm_bwd_reduce_x_typed(const void *dy, int dy_bf16, const void *x, int x_bf16, const float *scale, const float *shift, int batch, int c,
                                int64_t positions, float *sums, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_bncm_bwd_apply_x_typed(const void *dy, int dy_bf16, const void *x, int x_bf16, const float *scale, const float *shift, const float *a,
                               const float *b, const float *d, int batch, int c, int64_t positions, void *dx, int dx_bf16, s2d_stream_t stream);
int s2d_pcr_level_fwd_y16(const void *y, const float *bn_scale_shift, const float *head_params, const float *w2, const float *b2,
                          const int32_t *coors, const float *feats, int64_t m, int batch, int c, int co, int d, int h, int w, float *z,
                          float *z_stats, float *out8, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_pcr_level_bwd_sums_y16(const void *y, const float *bn_scale_shift, const float *head_params, const int32_t *coors, const float *feats,
                               int64_t m, int batch, int c, int d, int h, int w, const float *fwd_out8, const float *go_mask,
                               const float *go_offset, const float *dz, const float *w2, int co, float *grads, float *bn_sums, void *ws,
                               size_t ws_bytes, s2d_stream_t stream);
int s2d_pcr_level_bwd_apply_y16(const void *y, const float *bn_scale_shift, const float *head_params, const int32_t *coors, const float *feats,
                                int64_t m, int batch, int c, int d, int h, int w, const float *fwd_out8, const float *go_mask,
                                const float *go_offset, const float *dz, const float *w2, int co, const float *abd, float *dy,
                                s2d_stream_t stream);
/* bf16 y AND bf16 dy (the gradient's only readers, s2d_convt3d_mfma_{dgrad,wgrad}_d16, round it to bf16 anyway) */
int s2d_pcr_level_bwd_apply_y16_d16(const void *y, const float *bn_scale_shift, const float *head_params, const int32_t *coors, const float *feats,
                                    int64_t m, int batch, int c, int d, int h, int w, const float *fwd_out8, const float *go_mask,
                                    const float *go_offset, const float *dz, const float *w2, int co, const float *abd, void *dy_bf16,
                                    s2d_stream_t stream);

/* ---- fused PointPillars feature net (r04) ----------------------------------------------------------------------------------
 * One PFN layer of det3d/models/readers/pillar_encoder.py:41-56,114-154 (decorate -> Linear(10 -> 64) -> BatchNorm1d -> ReLU -> max over
 * the slots) from the raw pillars voxels[P][slots][5], num_points[P], coors[P][4] (b,z,y,x), recomputing the per-row products in every
 * pass instead of storing [P,slots,64] tensors.  _stats: per-workgroup partial slabs [s2d_pfn_blocks(P)][2][64] (fold with
 * s2d_bn_partials_sum_f32, n = P * slots rows).  _apply_max: out[P][64] and the slot of the maximum (uint8, first maximum).  _bwd: per-
 * workgroup rows of s2d_pfn_bwd_cols() floats: sum g[64] | sum g*h[64] | M1[10][64] | M2[10][64] | M3[10] (dout must already carry relu').
 */
int s2d_pfn_supported(int ndim, int slots, int feats, int cout);
int s2d_pfn_blocks(int64_t pillars);
int s2d_pfn_bwd_cols(void);
int s2d_pfn_stats_f32(const float *voxels, const int32_t *num_points, const int32_t *coors, const float *weight, int64_t pillars,
                      int slots, int ndim, float vx, float vy, float x_offset, float y_offset, float *partial, s2d_stream_t stream);
int s2d_pfn_apply_max_f32(const float *voxels, const int32_t *num_points, const int32_t *coors, const float *weight, const float *scale,
                          const float *shift, int64_t pillars, int slots, int ndim, float vx, float vy, float x_offset, float y_offset,
                          float *out, uint8_t *argmax, s2d_stream_t stream);
int s2d_pfn_bwd_f32(const float *voxels, const int32_t *num_points, const int32_t *coors, const float *weight, const float *dout,
                    const uint8_t *argmax, int64_t pillars, int slots, int ndim, float vx, float vy, float x_offset, float y_offset,
                    float *partial, s2d_stream_t stream);

/* Two PFN layers (the configs under configs/waymo/pp: num_filters = [64, 64]; layer 1 Linear(10 -> 32) -> BN -> ReLU -> [x | max over slots], layer 2
 * Linear(64 -> 64) -> BN -> ReLU -> max over slots; pillar_encoder.py:41-56).  scale_shift1 = scale[32] | shift[32] of the first batch
 * norm, scale_shift2 = scale[64] | shift[64] of the second.  _stats1 / _stats2: per-workgroup partial slabs [s2d_pfn_blocks(P)][2][64]
 * of (sum h, sum h^2) over the valid rows of layer 1 (columns 32..63 duplicate 0..31) / over all P*slots rows of layer 2.  _apply_max:
 * out[P][64], the slot of the maximum (first maximum; slot index num_points = an empty slot) and h2 at that slot.  _bwd: abd2 = a | b | d
 * of the second batch norm's backward (dh2 = a g + b h2 + d), gout = dout with relu' applied; writes s2d_pfn2_bwd_rows() rows of
 * s2d_pfn2_bwd_cols() floats: dW2[64][64] | sum g1[64] | sum g1 h1[64] | M1[10][64] | M2[10][64] | M3[10] (layer-1 entries in columns
 * 0..31), to be summed over the rows. */
int s2d_pfn2_supported(int ndim, int slots, int feats, int c1, int c2);
int s2d_pfn2_bwd_rows(void);
int s2d_pfn2_bwd_cols(void);
int s2d_pfn2_stats1_f32(const float *voxels, const int32_t *num_points, const int32_t *coors, const float *w1, int64_t pillars, int slots,
                        int ndim, float vx, float vy, float x_offset, float y_offset, float *partial, s2d_stream_t stream);
int s2d_pfn2_stats2_f32(const float *voxels, const int32_t *num_points, const int32_t *coors, const float *w1, const float *w2,
                        const float *scale_shift1, int64_t pillars, int slots, int ndim, float vx, float vy, float x_offset,
                        float y_offset, float *partial, s2d_stream_t stream);
int s2d_pfn2_apply_max_f32(const float *voxels, const int32_t *num_points, const int32_t *coors, const float *w1, const float *w2,
                           const float *scale_shift1, const float *scale_shift2, int64_t pillars, int slots, int ndim, float vx, float vy,
                           float x_offset, float y_offset, float *out, uint8_t *argmax, float *h2_at_max, s2d_stream_t stream);
int s2d_pfn2_bwd_f32(const float *voxels, const int32_t *num_points, const int32_t *coors, const float *w1, const float *w2,
                     const float *scale_shift1, const float *abd2, const float *gout, const uint8_t *argmax, int64_t pillars, int slots,
                     int ndim, float vx, float vy, float x_offset, float y_offset, float *partial, s2d_stream_t stream);

/*
 * Deformable convolution v1 (csrc/deform_conv.hip), the kernels behind CenterHead(dcn_head=True)'s FeatureAdaption
 * (det3d/models/bbox_heads/center_head.py:25-63).  Replaces det3d/ops/dcn: deform_conv_cuda.deform_conv_forward_cuda,
 * deform_conv_backward_input_cuda and deform_conv_backward_parameters_cuda (deform_conv.py DeformConvFunction; the im2col / col2im /
 * col2im_coord kernels of src/deform_conv_cuda_kernel.cu + GEMM).  No column buffer: the forward needs no workspace.
 * x, y, dy, y_saved, dx: bf16 NHWC.  offset / d_offset: NHWC [n][ho][wo][dg*2*kh*kw] in the reference's channel order (channel
 * g*2*kh*kw + 2*(i*kw+j) = row offset of tap (i, j), + 1 = column offset), fp32 (offset_bf16 = 0) or bf16 (1).  weight / dweight: fp32
 * [cout][cin][kh][kw]; the two packed images hold kh*kw*cin*cout bf16 each.
 * _supported: 1 for 64 -> 64, 3x3, stride 1, padding 1, dilation 1, groups 1, dg 4 - the shape the GPU suite runs the kernels at; 0
 * otherwise (the caller's composite path).  relu: ReLU fused into the forward epilogue; the backward entries take the saved OUTPUT as y_saved and
 * re-derive the mask from it (NULL: no ReLU).  _bwd_data: dx accumulates in the fp32 workspace (zeroed by a kernel, fp32 atomics), then
 * is stored as bf16; d_offset has one owner per element (deterministic).  _wgrad: per-workgroup partials in the workspace, folded in
 * a fixed order (deterministic).  Offsets may hold any value (NaN, Inf, +-1e6): positions outside the sampling window read and write
 * nothing.
 */
int s2d_deform_conv_supported(int cin, int cout, int kh, int kw, int stride, int pad, int dil, int groups, int dg);
size_t s2d_deform_conv_workspace_bytes(int n_img, int h, int w, int cin, int cout, int kh, int kw);
int s2d_deform_conv_pack_weights_bf16(const float *weight, int cin, int cout, int kh, int kw, void *packed_fwd, void *packed_bwd,
                                      s2d_stream_t stream);
int s2d_deform_conv_nhwc_bf16(const void *x, const void *offset, int offset_bf16, const void *packed_fwd, int n_img, int h, int w, int cin,
                              int cout, int kh, int kw, int stride, int pad, int dil, int dg, int relu, void *y, s2d_stream_t stream);
size_t s2d_deform_conv_bwd_data_workspace_bytes(int n_img, int h, int w, int cin);
int s2d_deform_conv_bwd_data_nhwc_bf16(const void *x, const void *offset, int offset_bf16, const void *dy, const void *y_saved,
                                       const void *packed_bwd, int n_img, int h, int w, int cin, int cout, int kh, int kw, int stride,
                                       int pad, int dil, int dg, void *dx, void *d_offset, void *ws, size_t ws_bytes, s2d_stream_t stream);
size_t s2d_deform_conv_wgrad_workspace_bytes(int n_img, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int dil);
int s2d_deform_conv_wgrad_nhwc_bf16(const void *x, const void *offset, int offset_bf16, const void *dy, const void *y_saved, int n_img,
                                    int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int dil, int dg, float *dweight,
                                    void *ws, size_t ws_bytes, s2d_stream_t stream);

/*
 * Two-stage RoI path on the device (csrc/roi_head.hip): what det3d/models/detectors/two_stage.py:50-199 does between the first stage's
 * predict and the RoI MLP, and behind the MLP at inference.  B samples, `cap` RoI slots per sample (NMS_POST_MAXSIZE); boxes are
 * (x, y, z, w, l, h, yaw).  Everything is fp32 in the torch chain's expression order; one launch per entry, no workspace.
 *
 * s2d_roi_pack (two_stage.py:76-122, reorder_first_stage_pred_and_feature without the features): the packed first-stage lists boxes
 * [total][box_dim] (heading LAST), scores [total], labels [total] int64, sample b's rows being offsets[b] .. offsets[b + 1] (HOST int32
 * [B + 1], B <= S2D_ROI_MAX_BATCH: they travel in the kernel arguments), become rois [B][cap][7], roi_scores [B][cap], roi_labels
 * [B][cap] int64 = label + 1; the slots behind a sample's rows are all zero (label 0), rows behind `cap` are dropped.
 *
 * s2d_roi_bev_features (two_stage.py:50-74 get_box_center, bird_eye_view.py:9-41, center_utils.py:93-122): feats [B][cap][num_point *
 * channels] fp32 = the bilinear samples of the map at the box centre (num_point 1) or at the centre and the four face centres
 * (num_point 5) of box row[b][slot], point 0's channels first; a -1 slot is written as zeros.  The map is read in place: element
 * (b, c, y, x) at b * stride_b + c * stride_c + y * stride_h + x * stride_w ELEMENTS from `map`, map_dtype 0 fp32 / 1 bf16 (widened
 * before the multiply).  Cell coordinate = (p - pc) / voxel / out_stride as two divisions; neighbours clamped to the map, weights from
 * the clamped neighbours, the four products summed in the reference's order.  Contiguous channels (stride_c 1, channels_last) with 16-byte
 * aligned rows take 16-byte loads; every other layout and channel count is read element by element.
 *
 * s2d_roi_match_gt (proposal_target_layer.py:74-104,208-237 over iou3d_nms_utils.py:28-70): gt [B][num_gt][gt_dim], the box in the
 * first 7 columns and the class in the LAST, num_gt <= S2D_ROI_MAX_GT.  Per sample the valid rows are 0 .. the last row whose fp32
 * column sum (all gt_dim columns, left to right) is not 0, at least row 0; gt_count [B] int32 = their number.  max_iou [B][cap] = the
 * largest 3-D IoU (rotated BEV overlap x height overlap / max(vol_a + vol_b - overlap, 1e-6)) of the RoI with the valid rows - with
 * by_class only rows whose class equals roi_labels - and assignment [B][cap] int64 = that row (the lowest on a tie); a RoI without a
 * row of its class gets 0 and row 0.
 *
 * s2d_roi_targets (ProposalTargetLayer.forward behind the sampling + RoIHead.assign_targets, roi_head_template.py:43-92): idx [B][per]
 * int32 = the sampled slots.  Gathers out_rois [B][per][7], out_labels int64, out_scores, out_iou, gt_of_rois_src [B][per][8] (7 box
 * columns + the class of row `assignment`), and writes gt_of_rois [B][per][8] (the residual in the RoI's frame: limit_period, the
 * subtraction, the rotation, the heading flip and clamp; the class column unchanged), reg_valid_mask int64 = iou > reg_fg_thresh, and
 * rcnn_cls_labels: cls_score_type 0 "cls" int64 (1 above cls_fg_thresh, -1 between the thresholds, else 0), 1 "roi_iou" fp32
 * (1 above, 0 below cls_bg_thresh, (iou - bg) / (fg - bg) between).  roi_dim must be 7.
 *
 * s2d_roi_refine (roi_head_template.py:153-183 generate_predicted_boxes + two_stage.py:124-150 post_process): n = B * cap RoIs;
 * boxes [n][7] = the residual rcnn_reg [n][7] plus the RoI's size and heading, rotated by its yaw and moved to its centre; scores [n] =
 * sqrt(sigmoid(rcnn_cls) * roi_score); labels [n] int64 = roi_label - 1 (-1 on the padding, which the caller slices off).
 *
 * The static forms read padded rows with DEVICE counts where they lie (center_predict.StaticDetections) and take no host table: launches
 * only, capturable into a HIP graph behind the static predict (second_stage.StaticRoIPlan).
 *
 * s2d_roi_pack_static: boxes [B][det_cap][7] (heading last), scores [B][det_cap], labels [B][det_cap] int64, counts [B] int32, all on the
 * device, 1 <= B <= S2D_ROI_MAX_BATCH, B * det_cap < 2^31.  With n_b = clamp(counts[b], 0, min(det_cap, cap)): slot i < n_b of sample b
 * gets rois [B][cap][7], roi_scores [B][cap], roi_labels [B][cap] int64 = label + 1 of input row (b, i) and row [B][cap] int32 =
 * b * det_cap + i; the slots >= n_b are all zero with label 0 and row -1 (as s2d_roi_pack pads); out_counts [B] int32 = n_b.  No input
 * row at or behind counts[b] is read.  `row` is the table s2d_roi_bev_features takes over `boxes` as the packed list [B * det_cap][7].
 *
 * s2d_roi_refine_static: s2d_roi_refine (the same device function) on [B][cap] with counts [B] int32 on the device: the rows < counts[b]
 * get its result, the rows >= counts[b] are WRITTEN as zero boxes, zero scores and label -1 and their inputs are not read - every output
 * element is a function of the rows below the counts alone.
 */
#define S2D_ROI_MAX_GT 512
#define S2D_ROI_MAX_BATCH 64
int s2d_roi_pack(const float *boxes, const float *scores, const int64_t *labels, int box_dim, const int32_t *offsets, int batch, int cap,
                 float *rois, float *roi_scores, int64_t *roi_labels, s2d_stream_t stream);
int s2d_roi_bev_features(const void *map, int map_dtype, int batch, int channels, int h, int w, int64_t stride_b, int64_t stride_c,
                         int64_t stride_h, int64_t stride_w, const float *boxes, int64_t total, int box_dim, const int32_t *row, int cap,
                         int num_point, float pc_x, float pc_y, float voxel_x, float voxel_y, float out_stride, float *feats,
                         s2d_stream_t stream);
int s2d_roi_match_gt(const float *rois, const int64_t *roi_labels, int batch, int cap, const float *gt, int num_gt, int gt_dim, int by_class,
                     float *max_iou, int64_t *assignment, int32_t *gt_count, s2d_stream_t stream);
int s2d_roi_targets(const int32_t *idx, int batch, int per, int cap, int roi_dim, const float *rois, const int64_t *roi_labels,
                    const float *roi_scores, const float *max_iou, const int64_t *assignment, const float *gt, int num_gt, int gt_dim,
                    double reg_fg_thresh, double cls_fg_thresh, double cls_bg_thresh, int cls_score_type, float *out_rois, int64_t *out_labels,
                    float *out_scores, float *out_iou, float *gt_of_rois_src, float *gt_of_rois, int64_t *reg_valid_mask,
                    void *rcnn_cls_labels, s2d_stream_t stream);
int s2d_roi_refine(const float *rois, const float *roi_scores, const int64_t *roi_labels, const float *rcnn_cls, const float *rcnn_reg,
                   int64_t n, float *boxes, float *scores, int64_t *labels, s2d_stream_t stream);
int s2d_roi_pack_static(const float *boxes, const float *scores, const int64_t *labels, const int32_t *counts, int batch, int det_cap,
                        int cap, float *rois, float *roi_scores, int64_t *roi_labels, int32_t *row, int32_t *out_counts,
                        s2d_stream_t stream);
int s2d_roi_refine_static(const float *rois, const float *roi_scores, const int64_t *roi_labels, const float *rcnn_cls,
                          const float *rcnn_reg, const int32_t *counts, int batch, int cap, float *boxes, float *scores, int64_t *labels,
                          s2d_stream_t stream);

/*
 * The eval-mode RoI MLP in one launch (csrc/roi_mlp.hip; roi_head.py:16-106, roi_head_template.py:27-41): feats [rows][cin] fp32
 * row-major and 16-byte aligned (what s2d_roi_bev_features writes) -> rcnn_cls [rows][1], rcnn_reg [rows][7].  Every layer is
 * y = act(scale[c] * (x . W^T)[c] + shift[c]) in exact fp32 on the matrix cores (v_mfma_f32_16x16x4_f32), scale and shift applied in the
 * epilogue: Conv1d(k=1, no bias) + eval BatchNorm1d + ReLU has scale = gamma / sqrt(running_var + eps), shift = beta - running_mean *
 * scale; the two final convolutions have scale 1, shift = bias and no ReLU; dropout is the identity.  No split-K, no atomics: a row's
 * result depends on that row only and is the same bits whatever else is in the call.
 *
 * Shape family (s2d_roi_mlp_supported): cin % 4 == 0, cin <= 4096; n_shared 1 or 2 layers of widths s0, s1; n_cls and n_reg 0, 1 or 2
 * hidden layers of widths c0, c1 / r0, r1; every hidden width a multiple of 16, at most 256 (widths behind a count are ignored);
 * num_class 1, code_size 7.  Anything else is S2D_ERR_UNSUPPORTED - the caller keeps the torch MLP.
 *
 * s2d_roi_mlp_plan_make fills the layer table, which then travels BY VALUE in the kernel arguments: layers in the order shared .., cls
 * hidden .., cls final, reg hidden .., reg final; cout_pad = cout for the hidden layers and 16 for the two final ones.
 *   image:  packed[w_off + (ks * (cout_pad / 16) + t) * 64 + l] = W[16 t + (l & 15)][4 ks + (l >> 4)]  (W [cout][cin] row-major, zero
 *           for rows past cout) - the B fragment of lane l for the 4-channel step ks and the 16-column tile t: one float per lane and
 *           instruction, 256 contiguous bytes per wave.  packed_elems floats in all (s2d_roi_mlp_packed_elems).
 *   affine: affine[affine_off + c] = scale[c], affine[affine_off + cout_pad + c] = shift[c], c < cout_pad (the padding is never read
 *           into a result); affine_elems floats in all.  The caller writes it.
 * s2d_roi_mlp_pack: one launch, weights = HOST array of num_layers device pointers in the table's order.
 */
#define S2D_ROI_MLP_MAX_LAYERS 8
typedef struct s2d_roi_mlp_layer {
    int32_t cin, cout, cout_pad, relu;
    int32_t affine_off, reserved;
    int64_t w_off;
} s2d_roi_mlp_layer;
typedef struct s2d_roi_mlp_plan {
    int32_t num_layers, n_shared, n_cls, n_reg;
    int64_t packed_elems;
    int32_t affine_elems, reserved;
    s2d_roi_mlp_layer layer[S2D_ROI_MLP_MAX_LAYERS];
} s2d_roi_mlp_plan;
int s2d_roi_mlp_supported(int cin, int n_shared, int s0, int s1, int n_cls, int c0, int c1, int n_reg, int r0, int r1, int num_class,
                          int code_size);
int64_t s2d_roi_mlp_packed_elems(int cin, int n_shared, int s0, int s1, int n_cls, int c0, int c1, int n_reg, int r0, int r1, int num_class,
                                 int code_size);
int s2d_roi_mlp_plan_make(int cin, int n_shared, int s0, int s1, int n_cls, int c0, int c1, int n_reg, int r0, int r1, int num_class,
                          int code_size, s2d_roi_mlp_plan *plan);
int s2d_roi_mlp_pack(const s2d_roi_mlp_plan *plan, const float *const *weights, float *packed, s2d_stream_t stream);
int s2d_roi_mlp_run(const s2d_roi_mlp_plan *plan, const float *feats, int64_t rows, const float *packed, const float *affine, float *rcnn_cls,
                    float *rcnn_reg, s2d_stream_t stream);

/*
 * The TRAINING branch of the same MLP (csrc/roi_mlp_train.hip): forward with batch statistics and caller-supplied dropout masks, the two RoI
 * losses, and the backward of all of it, fp32 on the matrix cores, one launch per depth (a batch norm couples all rows).  The plan and the
 * packed image are those of s2d_roi_mlp_plan_make / s2d_roi_mlp_pack; args holds, per layer of the plan's table, the UNPACKED weight
 * [cout][cin], then for a hidden layer gamma, beta, the running statistics (moved in place: momentum, unbiased variance), the 0/1 byte mask
 * [rows][cout] of the dropout site behind it (NULL: none) with keep_scale = 1 / (1 - p), and for a final layer its bias; the d_* pointers
 * receive the gradients (backward only).  Shape family: that of s2d_roi_mlp_supported, 2 <= rows <= 8192, dropout ratio < 1.
 * Hidden layer: z = a . W^T, mean / biased variance over the rows (per-tile mean and M2 merged in tile order with Chan's formula),
 * a' = relu(gamma * (z - mean) / sqrt(var + eps) + beta) * mask * keep_scale.  The features get no gradient.
 * The workspace (s2d_roi_mlp_train_scratch_bytes; 0 for a bad plan or row count) carries z, the statistics, dy and the per-tile backward
 * sums from the forward to the backward call; every word is written before it is read.  No atomics, no zero-fill: same inputs, same bits.
 * s2d_roi_mlp_train_launches: the kernel launches of one forward and one backward call.
 *
 * s2d_roi_loss_forward: out[0] = w_cls * sum over rows with labels >= 0 of BCE(sigmoid(rcnn_cls), labels) / max(valid, 1), logarithms
 * clamped at -100 as torch does; out[1] = w_reg * sum over rows with fg > 0 of |rcnn_reg - target| . code_weights / max(fg rows, 1);
 * out[2], out[3] = the two counts.  labels, fg [rows] fp32, target [rows][7]; code_weights = HOST array of 7.  s2d_roi_loss_backward:
 * torch's gradients of the two for the upstream DEVICE scalars g_cls, g_reg: (p - y) / max(p (1 - p), 1e-12) * p (1 - p) and sign().
 */
typedef struct s2d_roi_mlp_train_layer {
    const float *weight, *gamma, *beta;
    float *running_mean, *running_var;
    const float *bias;
    const uint8_t *mask;
    float *d_weight, *d_gamma, *d_beta, *d_bias;
    float keep_scale, momentum, eps;
    int32_t reserved;
} s2d_roi_mlp_train_layer;
typedef struct s2d_roi_mlp_train_args {
    s2d_roi_mlp_train_layer layer[S2D_ROI_MLP_MAX_LAYERS];
} s2d_roi_mlp_train_args;
int s2d_roi_mlp_train_supported(int cin, int n_shared, int s0, int s1, int n_cls, int c0, int c1, int n_reg, int r0, int r1, int num_class,
                                int code_size, int64_t rows, float dp_ratio);
size_t s2d_roi_mlp_train_scratch_bytes(const s2d_roi_mlp_plan *plan, int64_t rows);
int s2d_roi_mlp_train_launches(const s2d_roi_mlp_plan *plan, int *forward, int *backward);
int s2d_roi_mlp_train_forward(const s2d_roi_mlp_plan *plan, const s2d_roi_mlp_train_args *args, const float *feats, int64_t rows,
                              const float *packed, void *workspace, size_t workspace_bytes, float *rcnn_cls, float *rcnn_reg,
                              s2d_stream_t stream);
int s2d_roi_mlp_train_backward(const s2d_roi_mlp_plan *plan, const s2d_roi_mlp_train_args *args, const float *feats, int64_t rows,
                               void *workspace, size_t workspace_bytes, const float *d_rcnn_cls, const float *d_rcnn_reg, s2d_stream_t stream);
int s2d_roi_loss_forward(const float *rcnn_cls, const float *rcnn_reg, const float *labels, const float *fg, const float *target, int64_t rows,
                         const float *code_weights, float w_cls, float w_reg, float *out, s2d_stream_t stream);
int s2d_roi_loss_backward(const float *rcnn_cls, const float *rcnn_reg, const float *labels, const float *fg, const float *target, int64_t rows,
                          const float *code_weights, float w_cls, float w_reg, const float *out, const float *g_cls, const float *g_reg,
                          float *d_rcnn_cls, float *d_rcnn_reg, s2d_stream_t stream);

/*
 * Frame preparation of the S2D data step (csrc/prep.hip; det3d/datasets/pipelines/preprocess.py:81-117,178-201,257-260).  points
 * [n_points][ncols] and obj_points [obj_rows][ncols] fp32 with x, y, z first; boxes [num_boxes][box_dim] fp32 with the centre in
 * columns 0-2, the size in 3-5 and the yaw in the LAST column; num_boxes <= S2D_PREP_MAX_BOXES, row counts <= S2D_PREP_MAX_POINTS.
 *
 * Inside test (box_np_ops.py:641-647, geometry.py:215-276; strict on all six faces), fp32: with d = p - centre,
 *   |d.x cos r - d.y sin r| < dim0 / 2,  |d.x sin r + d.y cos r| < dim1 / 2,  |d.z| < dim2 / 2,
 * cos r and sin r evaluated in double from the fp32 yaw and rounded to fp32.
 *
 * s2d_prep_points_in_rbbox: mask [n_points][num_boxes] bytes (0 / 1) and / or counts [num_boxes] int32, either may be NULL (not both).
 *
 * s2d_prep_compose_count + s2d_prep_compose_fill (training mode, distillation): kinds [num_boxes] int8 (0 other, 1 VEHICLE, 2 SIGN);
 * obj_offsets [num_boxes + 1] int32 DEVICE array, the stored cloud of box j = rows obj_offsets[j] .. obj_offsets[j + 1] of obj_points
 * in the object's own frame (entries are clamped to 0 .. obj_rows on the device).  A box with an empty range, and every SIGN, takes the
 * frame's own points inside it.  A stored VEHICLE keeps the side y > 0 or y < 0 with strictly more points (a tie takes y < 0; y == 0
 * is dropped) and appends that side's mirror image; stored rows are rotated by pi / 2 + yaw about z (x' = x c + y s, y' = -x s + y c)
 * and moved to the box centre.  dense = the points outside every box in input order, then each box's block in box order (a point in
 * two boxes appears in both blocks); reconstruction = the blocks of the boxes that are no SIGN, in order, without the rows that lie
 * in no box of the frame.  _count runs four launches and leaves totals[0] = dense rows, totals[1] = reconstruction rows, totals[2] = the
 * number of boxes that are no SIGN (device int32[3], the one read the host needs); _fill, one launch, writes both clouds from the SAME workspace, untouched in between, and
 * never writes past dense_rows / recon_rows.
 *
 * s2d_prep_global_noise (core/sampler/preprocess.py:859-908,790-813,902-908,1032-1056): one launch over up to three clouds, columns
 * 0-2 in place: y = -y (flip_x), x = -x (flip_y), x' = x c + y s, y' = -x s + y c, all three times scale, then (translate != 0) plus
 * tx, ty, tz added in double.  The draws are the caller's.
 *
 * s2d_prep_gather_rows: dst[i] = src[perm[i]], perm [rows] int64 (the host's shuffle); dst must not alias src; a perm entry outside
 * 0 .. rows - 1 leaves its row unwritten.
 */
#define S2D_PREP_MAX_BOXES 512
#define S2D_PREP_MAX_POINTS (1 << 28)
size_t s2d_prep_workspace_bytes(int64_t n_points, int num_boxes, int64_t obj_rows);
int s2d_prep_points_in_rbbox(const float *points, int64_t n_points, int ncols, const float *boxes, int num_boxes, int box_dim, uint8_t *mask,
                             int32_t *counts, void *ws, size_t ws_bytes, s2d_stream_t stream);
int s2d_prep_compose_count(const float *points, int64_t n_points, int ncols, const float *boxes, int num_boxes, int box_dim,
                           const int8_t *kinds, const float *obj_points, int64_t obj_rows, const int32_t *obj_offsets, void *ws,
                           size_t ws_bytes, int32_t *totals, s2d_stream_t stream);
int s2d_prep_compose_fill(const float *points, int64_t n_points, int ncols, int num_boxes, const float *obj_points, int64_t obj_rows,
                          const void *ws, size_t ws_bytes, float *dense, int64_t dense_rows, float *recon, int64_t recon_rows,
                          s2d_stream_t stream);
int s2d_prep_global_noise(float *cloud0, int64_t rows0, float *cloud1, int64_t rows1, float *cloud2, int64_t rows2, int ncols, int flip_x,
                          int flip_y, float rot_cos, float rot_sin, float scale, int translate, double tx, double ty, double tz,
                          s2d_stream_t stream);
int s2d_prep_gather_rows(const float *src, int64_t rows, int ncols, const int64_t *perm, float *dst, s2d_stream_t stream);

/*
 * GT-database sampler of the training step (csrc/prep.hip, csrc/box_collision.h; det3d/core/sampler/sample_ops.py:134-359 and
 * box_collision_test of det3d/core/sampler/preprocess.py:922-1005, its `is True / is False` read by value: containment collides).
 *
 * s2d_prep_box_collision: out [n][k] bytes, out[i][j] = box_collision_test(corners, qcorners)[i][j]; corners [n][4][2] fp32.
 *
 * s2d_prep_gt_select (three launches): boxes [num_avoid + num_cand][box_dim], the frame's boxes first, then every group's candidates in
 * group order; group_ends HOST [num_groups], the exclusive end of each group's candidates; cand_meta DEVICE int32 [num_cand][5] = the
 * candidate's sweep rows [lo, hi) in src_points, its completed cloud's rows [lo, hi) in cc_points (empty: none; both clamped on the
 * device) and its kind (1 VEHICLE).  Candidates are walked in order; one is rejected when it collides with a frame box, an accepted
 * candidate, or a candidate of its own group that has not been rejected (later ones included).  header DEVICE int32 [2 + num_cand] =
 * accepted sweep rows, accepted reconstruction rows, accept[num_cand]: the step's one host read.  The reconstruction block of a candidate is
 * its completed cloud (VEHICLE: the side of y with strictly more rows, then its mirror image), rotated by pi / 2 + yaw, translated, and only
 * the rows strictly inside its own box; without a completed cloud, its translated sweep rows.
 * Limits: num_avoid + num_cand <= S2D_PREP_MAX_BOXES, 1 <= num_cand <= S2D_PREP_MAX_CANDIDATES, num_groups <= S2D_PREP_MAX_GROUPS;
 * s2d_prep_gt_scratch_bytes returns 0 outside them.
 *
 * s2d_prep_gt_paste (one launch, same ws and header): the accepted candidates' sweep rows with the box centre added to columns 0-2 into rows
 * 0 .. sampled_rows - 1 of points_out and of dense_out (may be NULL), their reconstruction blocks into rows 0 .. recon_rows - 1 of recon_out
 * (may be NULL with recon_rows 0).  Never writes past sampled_rows / recon_rows.
 */
#define S2D_PREP_MAX_CANDIDATES 128
#define S2D_PREP_MAX_GROUPS 16
size_t s2d_prep_gt_scratch_bytes(int num_avoid, int num_cand);
int s2d_prep_box_collision(const float *corners, int n, const float *qcorners, int k, uint8_t *out, s2d_stream_t stream);
int s2d_prep_gt_select(const float *boxes, int num_avoid, int num_cand, int box_dim, const int32_t *group_ends, int num_groups,
                       const int32_t *cand_meta, const float *cc_points, int64_t src_rows, int64_t cc_rows, int ncols, void *ws, size_t ws_bytes,
                       int32_t *header, s2d_stream_t stream);
int s2d_prep_gt_paste(int num_cand, int ncols, const int32_t *cand_meta, const float *src_points, int64_t src_rows, const float *cc_points,
                      int64_t cc_rows, const void *ws, size_t ws_bytes, const int32_t *header, float *points_out, float *dense_out,
                      int64_t sampled_rows, float *recon_out, int64_t recon_rows, s2d_stream_t stream);

/* ---- center-based multi-object tracker (csrc/tracking.hip): PubTracker.step_centertrack of the reference's tools/nusc_tracking and
 * tools/waymo_tracking behind transform_box, one workgroup per segment (sequence), every segment in ONE launch, nothing for the host to read.
 *
 * boxes [rows][9] fp32 in the lidar frame (centre 0-2, velocity 6-7), labels int64 [rows], scores fp32 [rows].  segments DEVICE
 * [num_segments]: pose = the first three rows of the 4x4 lidar-to-global matrix (row major), time_lag = this frame's timestamp minus the
 * previous one's, first != 0: the segment is reset before the step (tracks cleared, id_count 0), skip != 0: the segment's state is copied
 * to the new buffers bit for bit and its rows get tracking_id -1, [row_lo, row_hi) the segment's rows (clamped to 0 .. rows; at most
 * S2D_TRACK_MAX_DETS are used).  label_table DEVICE [num_labels]: the tracking class of a detection label (0 .. 126, or negative: the
 * label is not tracked) and its max_diff in metres.  score_thresh < 0: every unmatched detection starts a track (the nuScenes rule);
 * otherwise only those with score > score_thresh (fp32), the others are dropped (the Waymo rule).
 *
 * State per segment, capacity S2D_TRACK_MAX_TRACKS, read from the *_old buffers and written to the *_new ones (different buffers):
 * ct, tracking double [S][cap][2], meta int32 [S][cap][4] = class, id, age, active, head int32 [S][2] = count, id_count.  The new list
 * holds the matched detections in detection order (the track's id, age 1, active + 1), the unmatched ones (id = ++id_count, age 1, active
 * 1), then the unmatched old tracks with age < max_age in track order (age + 1, active 0, ct - tracking).  A segment without rows clears
 * its tracks and keeps id_count; with rows that are all filtered every track is unmatched and ages (the reference raises there).
 * tracking_id, active int32 [rows] in detection order: -1 / 0 for filtered or dropped rows. */
#define S2D_TRACK_MAX_SEGMENTS 64
#define S2D_TRACK_MAX_DETS 1024
#define S2D_TRACK_MAX_TRACKS 4096
typedef struct {
    double pose[12];
    double time_lag;
    int32_t first, skip, row_lo, row_hi;
} s2d_track_segment;
typedef struct {
    int32_t cls;
    float max_diff;
} s2d_track_label;
int s2d_track_step(const float *boxes, const int64_t *labels, const float *scores, int64_t rows, int num_segments,
                   const s2d_track_segment *segments, const s2d_track_label *label_table, int num_labels, int max_age, float score_thresh,
                   const double *ct_old, const double *tracking_old, const int32_t *meta_old, const int32_t *head_old, double *ct_new,
                   double *tracking_new, int32_t *meta_new, int32_t *head_new, int32_t *tracking_id, int32_t *active, s2d_stream_t stream);
/* The same step on padded, device-counted rows, for callers that must not touch the host between predict and track (the output of
 * s2d_predict_static_gather goes in as it lies) and for HIP-graph capture: ONE launch, the same association code.
 *
 * boxes [S][cap][9] fp32, labels int64 [S][cap], scores fp32 [S][cap], counts int32 [S] on the DEVICE: segment s owns rows
 * s * cap .. s * cap + clamp(counts[s], 0, cap) - 1 and nothing behind them is read.  frames DEVICE [S] (112 bytes each): pose as above,
 * stamp = this frame's timestamp in seconds, first, skip as above.  The time lag is formed on the device: first ? 0 : stamp - prev_stamp[s]
 * in double; prev_stamp double [S] is state and takes the new stamp unless skip is set.
 *
 * State: the layout above twice - ct, tracking double [2][S][S2D_TRACK_MAX_TRACKS][2], meta int32 [2][S][S2D_TRACK_MAX_TRACKS][4], head
 * int32 [2][S][2] - plus parity int32 [S]: half parity[s] holds segment s's current list; a step reads it, writes the other half and
 * stores parity[s] = 1 - parity[s].  A skipped segment keeps parity, state and prev_stamp untouched (no copy).  Zero everything once.
 * tracking_id, active int32 [S][cap]: all cap rows are written at every call, -1 / 0 for filtered rows, for rows at or behind counts[s]
 * and for every row of a skipped segment.  first, an empty frame (counts[s] == 0), the label table, score_thresh and max_age as above.
 * Returns -1 before any HIP call for S outside 1..64, cap outside 1..S2D_TRACK_MAX_DETS, cap * (max_age + 1) > S2D_TRACK_MAX_TRACKS
 * (a segment's tracks never exceed the rows of its last max_age + 1 frames), num_labels outside 1..127 and null pointers. */
typedef struct {
    double pose[12];
    double stamp;
    int32_t first, skip;
} s2d_track_frame;
int s2d_track_step_static(const float *boxes, const int64_t *labels, const float *scores, const int32_t *counts, int num_segments, int cap,
                          const s2d_track_frame *frames, const s2d_track_label *label_table, int num_labels, int max_age, float score_thresh,
                          double *ct, double *tracking, int32_t *meta, int32_t *head, int32_t *parity, double *prev_stamp,
                          int32_t *tracking_id, int32_t *active, s2d_stream_t stream);

/* ---- detection AP evaluation (csrc/eval_ap.hip): the reference's KITTI-protocol evaluator (det3d/datasets/kitti/eval.py,
 * det3d/datasets/utils/eval.py, rotate_iou_gpu_eval of det3d/ops/nms/nms_gpu.py), every frame of a split in ONE launch per entry.
 *
 * Rows of all frames are concatenated; det_off / gt_off DEVICE int32 [frames + 1] are the frames' row offsets and ov_off DEVICE int64
 * [frames + 1] the offsets of their overlaps, ov_off[f + 1] - ov_off[f] = nd_f * ng_f.  A frame's overlaps are fp32 [ng_f][nd_f] (ground
 * truth major).  At most S2D_EVAL_MAX_ROWS detections and as many ground-truth rows (DontCare included) per frame; the caller checks that.
 * det_box / gt_box double [rows][7] = location, dimensions, rotation; det_img / gt_img double [rows][4] image boxes; det_score double
 * [rows]; gt_occ_trunc double [rows][2] = occluded, truncated; det_name / gt_name int32 [rows]: the index of the lower-cased name in the
 * reference's class table (0 car .. 10 cyclist), 11 van, 12 person_sitting, 15 anything else, plus 256 for the exact names DontCare / ignore.
 *
 * s2d_eval_overlaps: metric 0 image-box IoU (computed in double), 1 BEV IoU (fp32, the plane without z_axis), 2 3-D IoU (fp32 BEV
 * intersection, the height term from z_axis / z_center in double), all rounded to fp32.
 * classes / difficulties: HOST arrays (class 0..10, difficulty 0..2); min_overlaps DEVICE double [num_classes][num_overlaps], >= 0; a work
 * item ("combination") is c = (class index * num_difficulties + difficulty index) * num_overlaps + overlap index.
 * s2d_eval_match: the first pass (compute_fp=False).  tp_scores double [combinations][total_gt]: the scores of a frame's true positives in
 * ground-truth order from [c][gt_off[f]]; counts int32 [frames][combinations][2] = true positives, ground truths that count; pr (the
 * buffer of s2d_eval_pr) is cleared.
 * s2d_eval_pr: the second pass (compute_fp=True) at thresholds DEVICE double [combinations][S2D_EVAL_SAMPLE_PTS], the first
 * num_thresholds[c] of each; pr int64 [combinations][S2D_EVAL_SAMPLE_PTS][3] += tp, fp (after the DontCare subtraction of metric 0), fn
 * over the frames: integer sums, the same bits on every call. */
#define S2D_EVAL_MAX_ROWS 1024
#define S2D_EVAL_MAX_CLASSES 11
#define S2D_EVAL_SAMPLE_PTS 41
int s2d_eval_overlaps(int metric, const double *det_box, const double *det_img, const double *gt_box, const double *gt_img,
                      const int32_t *det_off, const int32_t *gt_off, const int64_t *ov_off, int frames, int64_t pairs, int z_axis,
                      double z_center, float *overlaps, s2d_stream_t stream);
int s2d_eval_match(const float *overlaps, const double *det_img, const double *det_score, const int32_t *det_name, const double *gt_img,
                   const double *gt_occ_trunc, const int32_t *gt_name, const int32_t *det_off, const int32_t *gt_off, const int64_t *ov_off,
                   int frames, const int32_t *classes, int num_classes, const int32_t *difficulties, int num_difficulties,
                   const double *min_overlaps, int num_overlaps, int64_t total_gt, double *tp_scores, int32_t *counts, int64_t *pr,
                   s2d_stream_t stream);
int s2d_eval_pr(const float *overlaps, const double *det_img, const double *det_score, const int32_t *det_name, const double *gt_img,
                const double *gt_occ_trunc, const int32_t *gt_name, const int32_t *det_off, const int32_t *gt_off, const int64_t *ov_off,
                int frames, int metric, const int32_t *classes, int num_classes, const int32_t *difficulties, int num_difficulties,
                const double *min_overlaps, int num_overlaps, const double *thresholds, const int32_t *num_thresholds, int64_t *pr,
                s2d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* S2D_H_ */
