// Rotated bird's-eye-view IoU and greedy NMS of CenterHead.predict:
//   box_torch_ops.rotate_nms_pcdet            /root/reference/det3d/core/bbox/box_torch_ops.py:449-464
//   iou3d_nms_cuda.nms_gpu / nms_kernel       /root/reference/det3d/ops/iou3d_nms/src/iou3d_nms_kernel.cu:236-326, src/iou3d_nms.cpp:92-130
// Boxes are 7 floats (x, y, z, dx, dy, dz, heading), already sorted by descending score.  Same geometry as the reference: the
// overlap polygon of two rotated rectangles is collected from (i) the proper intersections of the 4 x 4 edge pairs and (ii) the
// corners of either box lying inside the other (with its 1e-2 margin), ordered by angle around their centroid, and measured by
// the shoelace sum; IoU = overlap / max(area_a + area_b - overlap, 1e-8); box j is suppressed by an earlier kept box i when
// IoU(i, j) > threshold.
// Design: one kernel fills the upper-triangular suppression bit matrix (64 x 64 tiles, column boxes staged in LDS), a second,
// single-workgroup kernel walks it on the DEVICE (the reference copies the matrix to the host and walks it there) and writes
// the kept indices + their count: no host round trip inside predict().
#include "nms_geom.h"

namespace s2d {

__global__ __launch_bounds__(256) void bev_iou_matrix_kernel(const float *__restrict__ a, int na, const float *__restrict__ b, int nb, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)na * nb) return;
    out[i] = bev_iou(a + (i / nb) * 7, b + (i % nb) * 7);
}

// suppression bits: mask[i][cb] bit j = IoU(box i, box cb*64+j) > thresh, for j > i only (earlier boxes cannot be suppressed by later)
__global__ __launch_bounds__(64) void nms_mask_kernel(const float *__restrict__ boxes, int n, float thresh, unsigned long long *__restrict__ mask) {
    __shared__ float col[64 * 7];
    const int rb = blockIdx.y, cb = blockIdx.x;
    const int col_blocks = (n + 63) / 64;
    const int t = threadIdx.x;
    if (cb < rb) {   // strictly lower tiles carry no bits
        if (rb * 64 + t < n) mask[(int64_t)(rb * 64 + t) * col_blocks + cb] = 0ull;
        return;
    }
    const int cj = cb * 64 + t;
    if (cj < n)
        for (int e = 0; e < 7; ++e) col[t * 7 + e] = boxes[(int64_t)cj * 7 + e];
    __syncthreads();
    const int ri = rb * 64 + t;
    if (ri >= n) return;
    const float *mine = boxes + (int64_t)ri * 7;
    const int ncol = min(64, n - cb * 64);
    unsigned long long bits = 0ull;
    for (int j = (rb == cb ? t + 1 : 0); j < ncol; ++j)
        if (bev_iou(mine, col + j * 7) > thresh) bits |= 1ull << j;
    mask[(int64_t)ri * col_blocks + cb] = bits;
}

// centre-distance suppression bits (CenterPoint's circle NMS, det3d/core/utils/circle_nms_jit.py:4-31): bit j = (xi - xj)^2 + (yi - yj)^2 <= thresh
// (the reference compares the SQUARED distance with `min_radius` as is), j > i only
__global__ __launch_bounds__(64) void circle_mask_kernel(const float *__restrict__ xy, int n, float thresh, unsigned long long *__restrict__ mask) {
    __shared__ float col[64 * 2];
    const int rb = blockIdx.y, cb = blockIdx.x;
    const int col_blocks = (n + 63) / 64;
    const int t = threadIdx.x;
    if (cb < rb) {
        if (rb * 64 + t < n) mask[(int64_t)(rb * 64 + t) * col_blocks + cb] = 0ull;
        return;
    }
    const int cj = cb * 64 + t;
    if (cj < n) {
        col[t * 2] = xy[(int64_t)cj * 2];
        col[t * 2 + 1] = xy[(int64_t)cj * 2 + 1];
    }
    __syncthreads();
    const int ri = rb * 64 + t;
    if (ri >= n) return;
    const float x = xy[(int64_t)ri * 2], y = xy[(int64_t)ri * 2 + 1];
    const int ncol = min(64, n - cb * 64);
    unsigned long long bits = 0ull;
    for (int j = (rb == cb ? t + 1 : 0); j < ncol; ++j) {
        const float dx = x - col[j * 2], dy = y - col[j * 2 + 1];
        // the reference's expression, evaluated without FMA contraction (the library is built with -ffp-contract=off): (dx)**2 + (dy)**2
        if (dx * dx + dy * dy <= thresh) bits |= 1ull << j;
    }
    mask[(int64_t)ri * col_blocks + cb] = bits;
}

// greedy walk over the bit matrix in one workgroup: `removed` lives in LDS; box i is kept iff its bit is clear when reached
__global__ __launch_bounds__(256) void nms_select_kernel(const unsigned long long *__restrict__ mask, int n, int max_keep, int64_t *__restrict__ keep,
                                                         int32_t *__restrict__ n_keep) {
    extern __shared__ unsigned long long removed[];
    const int col_blocks = (n + 63) / 64;
    for (int e = threadIdx.x; e < col_blocks; e += 256) removed[e] = 0ull;
    __shared__ int count;
    __shared__ int alive;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        if (threadIdx.x == 0) alive = !((removed[i >> 6] >> (i & 63)) & 1ull);
        __syncthreads();
        if (alive) {
            if (threadIdx.x == 0) {
                if (count < max_keep) keep[count] = i;
                ++count;
            }
            for (int e = (i >> 6) + threadIdx.x; e < col_blocks; e += 256) removed[e] |= mask[(int64_t)i * col_blocks + e];
        }
        __syncthreads();
        if (count >= max_keep) break;   // uniform: count is shared and settled by the barrier
    }
    if (threadIdx.x == 0) n_keep[0] = count < max_keep ? count : max_keep;
}

}  // namespace s2d

using namespace s2d;

extern "C" int s2d_bev_iou_f32(const float *boxes_a, int na, const float *boxes_b, int nb, float *iou, s2d_stream_t stream) {
    S2D_CHECK_ARG(na >= 0 && nb >= 0, "bev_iou: bad sizes");
    if (na == 0 || nb == 0) return S2D_OK;
    S2D_CHECK_ARG(boxes_a && boxes_b && iou, "bev_iou: null argument");
    hipLaunchKernelGGL(bev_iou_matrix_kernel, dim3((unsigned)ceil_div((int64_t)na * nb, 256)), dim3(256), 0, (hipStream_t)stream, boxes_a, na, boxes_b,
                       nb, iou);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" size_t s2d_nms_workspace_bytes(int n) { return n <= 0 ? 256 : align_up((size_t)n * ((n + 63) / 64) * sizeof(unsigned long long), 256); }

extern "C" int s2d_nms_rotated_bev(const float *boxes_sorted, int n, float iou_threshold, int max_keep, int64_t *keep, int32_t *n_keep, void *ws,
                                   size_t ws_bytes, s2d_stream_t stream) {
    S2D_CHECK_ARG(n >= 0 && n <= 65536 && max_keep >= 0 && keep && n_keep, "nms: bad argument (n <= 65536)");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || max_keep == 0) {
        S2D_HIP(hipMemsetAsync(n_keep, 0, sizeof(int32_t), st));
        return S2D_OK;
    }
    S2D_CHECK_ARG(boxes_sorted, "nms: null boxes");
    if (!ws || ws_bytes < s2d_nms_workspace_bytes(n)) {
        set_error("nms: workspace too small");
        return S2D_ERR_WORKSPACE;
    }
    const int cb = (n + 63) / 64;
    unsigned long long *mask = (unsigned long long *)ws;
    hipLaunchKernelGGL(nms_mask_kernel, dim3(cb, cb), dim3(64), 0, st, boxes_sorted, n, iou_threshold, mask);
    hipLaunchKernelGGL(nms_select_kernel, dim3(1), dim3(256), (size_t)cb * sizeof(unsigned long long), st, mask, n, max_keep, keep, n_keep);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

/* CenterPoint's circle NMS (see include/s2d.h) */
extern "C" int s2d_nms_circle(const float *xy_sorted, int n, float thresh, int max_keep, int64_t *keep, int32_t *n_keep, void *ws, size_t ws_bytes,
                              s2d_stream_t stream) {
    S2D_CHECK_ARG(n >= 0 && n <= 65536 && max_keep >= 0 && keep && n_keep, "nms_circle: bad argument (n <= 65536)");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || max_keep == 0) {
        S2D_HIP(hipMemsetAsync(n_keep, 0, sizeof(int32_t), st));
        return S2D_OK;
    }
    S2D_CHECK_ARG(xy_sorted, "nms_circle: null centres");
    if (!ws || ws_bytes < s2d_nms_workspace_bytes(n)) {
        set_error("nms_circle: workspace too small");
        return S2D_ERR_WORKSPACE;
    }
    const int cb = (n + 63) / 64;
    unsigned long long *mask = (unsigned long long *)ws;
    hipLaunchKernelGGL(circle_mask_kernel, dim3(cb, cb), dim3(64), 0, st, xy_sorted, n, thresh, mask);
    hipLaunchKernelGGL(nms_select_kernel, dim3(1), dim3(256), (size_t)cb * sizeof(unsigned long long), st, mask, n, max_keep, keep, n_keep);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
