// Two-stage RoI path on the device (det3d/models/detectors/two_stage.py:50-199, second_stage/bird_eye_view.py:9-41,
// roi_heads/target_assigner/proposal_target_layer.py:14-237, roi_heads/roi_head_template.py:43-92,153-183): what sits between
// CenterHead.predict and the RoI MLP, and behind the MLP at inference, in five launches instead of a torch chain per sample.
//   roi_pack_kernel          packed first-stage lists -> the zero-padded [B, cap] RoI tensors (labels + 1, padding label 0); the
//                            per-sample offsets are host values and travel in the kernel arguments
//   roi_bev_features_kernel  five-point (or one-point) bilinear BEV features, the neck map read where it lies (fp32 / bf16, any strides)
//   roi_match_gt_kernel      best 3-D IoU and its ground-truth row for every RoI of every sample (bev_overlap of nms_geom.h directly)
//   roi_targets_kernel       gather of the sampled RoIs + residual targets in the RoI's frame + reg mask + classification labels
//   roi_refine_kernel        generate_predicted_boxes + the arithmetic of post_process
// and the two forms that read padded rows with DEVICE counts where they lie (StaticDetections), launches only, so that predict_static +
// second stage can be captured into one HIP graph:
//   roi_pack_static_kernel   padded [B, det_cap] detections + counts [B] -> the [B, cap] RoI tensors, the row table and the clamped counts
//   roi_refine_static_kernel roi_refine_kernel's arithmetic (the same device function) on the rows below counts[b], zeros / -1 behind them
// Expression order follows the torch chain on fp32 (the library is built with -ffp-contract=off): divisions are divisions, python
// scalars enter as their fp32 rounding.  Built without the SLP vectoriser (DESIGN rule 36): the file has fp32 blends and runs inside
// two-stage training beside the weight-gradient stream.
#include "nms_geom.h"

#include <limits.h>
#include <math.h>

namespace s2d {

constexpr int ROI_MAX_GT = S2D_ROI_MAX_GT;

constexpr int ROI_MAX_BATCH = S2D_ROI_MAX_BATCH;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// first row of every sample in the packed lists (and the total behind the last): travels by value in the kernel arguments
struct PackOffsets {
    int32_t at[ROI_MAX_BATCH + 1];
};

__global__ __launch_bounds__(256) void roi_pack_kernel(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                       const int64_t *__restrict__ labels, int box_dim, PackOffsets off, int cap,
                                                       float *__restrict__ rois, float *__restrict__ roi_scores,
                                                       int64_t *__restrict__ roi_labels) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;   // (b is block-uniform: the offsets are read from the arguments)
    if (i >= cap) return;
    const int64_t s = (int64_t)b * cap + i, r = (int64_t)off.at[b] + i;
    const bool valid = r < off.at[b + 1];
    const float *bx = boxes + (valid ? r : 0) * box_dim;
    for (int e = 0; e < 6; ++e) rois[s * 7 + e] = valid ? bx[e] : 0.f;
    rois[s * 7 + 6] = valid ? bx[box_dim - 1] : 0.f;
    roi_scores[s] = valid ? scores[r] : 0.f;
    roi_labels[s] = valid ? labels[r] + 1 : 0;
}

// The padded form: sample b's detections are the first counts[b] rows of boxes [B][det_cap][7] (scores, labels [B][det_cap]); the count is
// read on the device and clamped to what both sides hold.  Nothing at or behind the count is read: the padding may hold anything.  row is the
// table s2d_roi_bev_features takes over the boxes viewed as [B * det_cap][7].
__global__ __launch_bounds__(256) void roi_pack_static_kernel(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                              const int64_t *__restrict__ labels, const int32_t *__restrict__ counts,
                                                              int det_cap, int cap, float *__restrict__ rois, float *__restrict__ roi_scores,
                                                              int64_t *__restrict__ roi_labels, int32_t *__restrict__ row,
                                                              int32_t *__restrict__ out_counts) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = clampi(counts[b], 0, det_cap < cap ? det_cap : cap);
    if (i == 0) out_counts[b] = n;
    if (i >= cap) return;
    const int64_t s = (int64_t)b * cap + i, r = (int64_t)b * det_cap + i;
    if (i < n) {
        for (int e = 0; e < 7; ++e) rois[s * 7 + e] = boxes[r * 7 + e];
        roi_scores[s] = scores[r];
        roi_labels[s] = labels[r] + 1;
        row[s] = (int32_t)r;
        return;
    }
    for (int e = 0; e < 7; ++e) rois[s * 7 + e] = 0.f;   // (no load on this side: the padding of the inputs is never touched)
    roi_scores[s] = 0.f;
    roi_labels[s] = 0;
    row[s] = -1;
}

// ---- BEV features -----------------------------------------------------------------------------------------------------------------------
struct FeatArgs {
    const void *map;
    int channels, h, w;
    int64_t sb, sc, sh, sw;
    const float *boxes;
    int64_t total;
    int box_dim;
    const int32_t *row;
    int cap, num_point;
    int64_t pairs;   // batch * cap * num_point
    float pc_x, pc_y, voxel_x, voxel_y, out_stride;
    float *feats;
};

typedef unsigned short roi_us8 __attribute__((ext_vector_type(8)));
typedef float roi_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(unsigned short v) { return __uint_as_float((unsigned)v << 16); }   // bf16 -> fp32, exact

// floor of a map coordinate as an int that is safe to clamp: NaN and anything below -2 become -2, anything above `size` becomes `size`;
// after the clamp of x0 and x0 + 1 to [0, size - 1] that is what floor().long().clamp() gives
__device__ __forceinline__ int cell_of(float v, int size) { return (int)fminf(fmaxf(floorf(v), -2.f), (float)size); }

// the sample point `p` of box bx (two_stage.py:50-74 over box_torch_ops.center_to_corner_box2d / rotation_2d): 0 the centre, 1..4 the
// middles of the corner pairs (0, 1), (2, 3), (0, 3), (1, 2); corners clockwise from the minimum point
__device__ __forceinline__ void side_point(const float *bx, int box_dim, int p, float &px, float &py) {
    if (p == 0) {
        px = bx[0];
        py = bx[1];
        return;
    }
    const float s = sinf(bx[box_dim - 1]), c = cosf(bx[box_dim - 1]);
    const int ka = (p == 1 || p == 3) ? 0 : (p == 2 ? 2 : 1), kb = p == 1 ? 1 : (p == 4 ? 2 : 3);
    float x[2], y[2];
    for (int i = 0; i < 2; ++i) {
        const int k = i == 0 ? ka : kb;
        const float cx = bx[3] * (k >= 2 ? 0.5f : -0.5f), cy = bx[4] * (k == 1 || k == 2 ? 0.5f : -0.5f);
        x[i] = (cx * c + cy * s) + bx[0];
        y[i] = (-cx * s + cy * c) + bx[1];
    }
    px = (x[0] + x[1]) / 2;
    py = (y[0] + y[1]) / 2;
}

// One wave per (slot, point): the four tap rows and the four weights are wave-uniform, lanes run over the channels.  VEC = 8 (bf16) /
// 4 (fp32): channels are contiguous (stride 1) and every tap row is 16-byte aligned - one 16-byte load per lane and tap; VEC = 1: any
// strides, any channel count.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void roi_bev_features_kernel(FeatArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + wave;
    if (pair >= a.pairs) return;
    const int p = (int)(pair % a.num_point);
    const int64_t slot = pair / a.num_point;
    const int b = (int)(slot / a.cap), C = a.channels;
    float *out = a.feats + pair * C;
    const int r = a.row[slot];
    if (r < 0 || r >= a.total) {   // an empty slot: zeros, so that the output needs no separate fill
        if constexpr (VEC > 1) {
            const roi_f4 z = {0.f, 0.f, 0.f, 0.f};
            for (int c = lane * 4; c < C; c += 256) *(roi_f4 *)(out + c) = z;
        } else {
            for (int c = lane; c < C; c += 64) out[c] = 0.f;
        }
        return;
    }
    float px, py;
    side_point(a.boxes + (int64_t)r * a.box_dim, a.box_dim, p, px, py);
    const float x = (px - a.pc_x) / a.voxel_x / a.out_stride, y = (py - a.pc_y) / a.voxel_y / a.out_stride;
    const int x0 = cell_of(x, a.w), y0 = cell_of(y, a.h);
    const int x0c = clampi(x0, 0, a.w - 1), x1c = clampi(x0 + 1, 0, a.w - 1), y0c = clampi(y0, 0, a.h - 1), y1c = clampi(y0 + 1, 0, a.h - 1);
    // the weights come from the CLAMPED neighbours (center_utils.py:110-113): outside the map they are the reference's, not zero
    const float wa = ((float)x1c - x) * ((float)y1c - y), wb = ((float)x1c - x) * (y - (float)y0c);
    const float wc = (x - (float)x0c) * ((float)y1c - y), wd = (x - (float)x0c) * (y - (float)y0c);
    const T *base = (const T *)a.map + (int64_t)b * a.sb;
    const T *ta = base + y0c * a.sh + x0c * a.sw, *tb = base + y1c * a.sh + x0c * a.sw;
    const T *tc = base + y0c * a.sh + x1c * a.sw, *td = base + y1c * a.sh + x1c * a.sw;
    if constexpr (VEC == 8) {
        for (int c = lane * 8; c < C; c += 512) {
            const roi_us8 va = *(const roi_us8 *)(ta + c), vb = *(const roi_us8 *)(tb + c), vc = *(const roi_us8 *)(tc + c),
                          vd = *(const roi_us8 *)(td + c);
            roi_f4 lo, hi;
            for (int j = 0; j < 4; ++j) {
                lo[j] = widen(va[j]) * wa + widen(vb[j]) * wb + widen(vc[j]) * wc + widen(vd[j]) * wd;
                hi[j] = widen(va[j + 4]) * wa + widen(vb[j + 4]) * wb + widen(vc[j + 4]) * wc + widen(vd[j + 4]) * wd;
            }
            *(roi_f4 *)(out + c) = lo;
            *(roi_f4 *)(out + c + 4) = hi;
        }
    } else if constexpr (VEC == 4) {
        for (int c = lane * 4; c < C; c += 256) {
            const roi_f4 va = *(const roi_f4 *)(ta + c), vb = *(const roi_f4 *)(tb + c), vc = *(const roi_f4 *)(tc + c),
                         vd = *(const roi_f4 *)(td + c);
            roi_f4 o;
            for (int j = 0; j < 4; ++j) o[j] = va[j] * wa + vb[j] * wb + vc[j] * wc + vd[j] * wd;
            *(roi_f4 *)(out + c) = o;
        }
    } else {
        for (int c = lane; c < C; c += 64) {
            const int64_t o = c * a.sc;
            out[c] = widen(ta[o]) * wa + widen(tb[o]) * wb + widen(tc[o]) * wc + widen(td[o]) * wd;
        }
    }
}

// ---- IoU match ----------------------------------------------------------------------------------------------------------------------------
// (x, y, z, w, l, h, yaw) -> (x, y, z, dx, dy, dz, heading) of iou3d_nms_utils.py:22-26
__device__ __forceinline__ void to_pcdet(const float *src, float yaw, float *dst) {
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    dst[3] = src[4];
    dst[4] = src[3];
    dst[5] = src[5];
    dst[6] = -yaw - 1.5707964f;
}

// boxes_iou3d_gpu (iou3d_nms_utils.py:28-70) of two pcdet boxes.  A pair whose height ranges do not meet, or whose centres are further
// apart than the two half diagonals and the 1e-2 margin of inside_rect allow, has overlap 0 exactly: the polygon clip is skipped.
// the polygon points of one lane's clip: point i of thread t at spts[i * 256 + t] - dynamically indexed, so kept in LDS, not scratch
struct LanePoints {
    P2 *base;
    __device__ __forceinline__ P2 &operator[](int i) const { return base[(i < 16 ? i : 15) * 256]; }   // (two rectangles give at most 16)
};

__device__ __forceinline__ float iou3d_pair(const float *a, const float *b, const LanePoints &pts) {
    const float oh = fmaxf(fminf(a[2] + a[5] / 2, b[2] + b[5] / 2) - fmaxf(a[2] - a[5] / 2, b[2] - b[5] / 2), 0.f);
    const float dx = a[0] - b[0], dy = a[1] - b[1];
    const float reach = 0.5f * (sqrtf(a[3] * a[3] + a[4] * a[4]) + sqrtf(b[3] * b[3] + b[4] * b[4])) + 0.1f;
    float ov = 0.f;
    if (oh > 0.f && !(dx * dx + dy * dy > reach * reach)) ov = bev_overlap_with(a, b, pts) * oh;
    const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
    return ov / fmaxf(va + vb - ov, 1e-6f);
}

constexpr int MATCH_ROIS_PER_WAVE = 2, MATCH_ROIS_PER_BLOCK = 4 * MATCH_ROIS_PER_WAVE;

__global__ __launch_bounds__(256) void roi_match_gt_kernel(const float *__restrict__ rois, const int64_t *__restrict__ roi_labels, int cap,
                                                           const float *__restrict__ gt, int num_gt, int gt_dim, int by_class,
                                                           float *__restrict__ max_iou, int64_t *__restrict__ assignment,
                                                           int32_t *__restrict__ gt_count) {
    __shared__ float sbox[ROI_MAX_GT * 7];
    __shared__ int scls[ROI_MAX_GT];
    __shared__ P2 spts[16 * 256];
    __shared__ int last;
    const int b = blockIdx.y, tid = threadIdx.x;
    const LanePoints pts{spts + tid};
    const float *g = gt + (int64_t)b * num_gt * gt_dim;
    if (tid == 0) last = 0;
    __syncthreads();
    // the valid rows are 0 .. the last row whose column sum is not 0 (proposal_target_layer.py:85-89; row 0 always stays)
    for (int r = tid; r < num_gt; r += 256) {
        float sum = g[(int64_t)r * gt_dim];
        for (int e = 1; e < gt_dim; ++e) sum = sum + g[(int64_t)r * gt_dim + e];
        if (sum != 0.f) atomicMax(&last, r);
    }
    __syncthreads();
    const int count = last + 1;
    if (blockIdx.x == 0 && tid == 0) gt_count[b] = count;
    for (int r = tid; r < count; r += 256) {
        const float *src = g + (int64_t)r * gt_dim;
        to_pcdet(src, src[6], sbox + r * 7);
        scls[r] = (int)fminf(fmaxf(src[gt_dim - 1], -1e9f), 1e9f);   // .long() truncates
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int k = 0; k < MATCH_ROIS_PER_WAVE; ++k) {
        const int i = blockIdx.x * MATCH_ROIS_PER_BLOCK + wave * MATCH_ROIS_PER_WAVE + k;
        if (i >= cap) break;   // wave-uniform
        const int64_t slot = (int64_t)b * cap + i;
        float a[7];
        to_pcdet(rois + slot * 7, rois[slot * 7 + 6], a);
        const int64_t label = roi_labels[slot];
        float best = -1.f;
        int arg = INT_MAX;
        for (int r = lane; r < count; r += 64) {
            if (by_class && (int64_t)scls[r] != label) continue;
            const float v = iou3d_pair(a, sbox + r * 7, pts);
            if (arg == INT_MAX || v > best) {   // strict: rows come in ascending order, the lowest index wins a tie
                best = v;
                arg = r;
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(best, off);
            const int oa = __shfl_xor(arg, off);
            if (oa != INT_MAX && (arg == INT_MAX || ov > best || (ov == best && oa < arg))) {
                best = ov;
                arg = oa;
            }
        }
        if (lane == 0) {   // no row of the RoI's class: IoU 0 with row 0, what the reference's zero-initialised outputs hold
            max_iou[slot] = arg == INT_MAX ? 0.f : best;
            assignment[slot] = arg == INT_MAX ? 0 : arg;
        }
    }
}

// ---- targets ------------------------------------------------------------------------------------------------------------------------------
struct TargetArgs {
    const int32_t *idx;
    int64_t n;   // batch * per
    int per, cap, num_gt, gt_dim;
    const float *rois, *roi_scores, *max_iou, *gt;
    const int64_t *roi_labels, *assignment;
    float reg_fg, cls_fg, cls_bg, cls_span;
    int soft;   // CLS_SCORE_TYPE: 0 "cls" (int64 labels, -1 = ignored), 1 "roi_iou" (fp32 soft labels)
    float *out_rois, *out_scores, *out_iou, *gt_src, *gt_enc;
    int64_t *out_labels, *reg_valid;
    void *cls_labels;
};

// python's float modulo by a positive period, as torch.remainder
__device__ __forceinline__ float pymod(float v, float period) {
    float r = fmodf(v, period);
    if (r != 0.f && r < 0.f) r = r + period;
    return r;
}

__global__ __launch_bounds__(256) void roi_targets_kernel(TargetArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const int b = (int)(t / a.per);
    const int i = clampi(a.idx[t], 0, a.cap - 1);
    const int64_t slot = (int64_t)b * a.cap + i;
    const float *roi = a.rois + slot * 7;
    const int64_t row = a.assignment[slot];
    const float *g = a.gt + ((int64_t)b * a.num_gt + (row < 0 ? 0 : (row >= a.num_gt ? a.num_gt - 1 : row))) * a.gt_dim;
    const float iou = a.max_iou[slot];
    float src[8], r[7];
    for (int e = 0; e < 7; ++e) {
        r[e] = roi[e];
        src[e] = g[e];
        a.out_rois[t * 7 + e] = r[e];
    }
    src[7] = g[a.gt_dim - 1];
    for (int e = 0; e < 8; ++e) a.gt_src[t * 8 + e] = src[e];
    a.out_labels[t] = a.roi_labels[slot];
    a.out_scores[t] = a.roi_scores[slot];
    a.out_iou[t] = iou;
    // roi_head_template.py:57-92: the residual in the RoI's frame
    const float two_pi = 6.2831855f, pi = 3.1415927f;
    const float ry = r[6] - floorf(r[6] / two_pi + 0.5f) * two_pi;   // limit_period(offset 0.5, period 2 pi)
    float d[7];
    for (int e = 0; e < 6; ++e) d[e] = src[e] - r[e];
    d[6] = src[6] - ry;
    const float ca = cosf(-ry), sa = sinf(-ry);
    const float x = d[0] * ca + d[1] * sa, y = -d[0] * sa + d[1] * ca;
    float h = pymod(d[6], two_pi);
    if (h > 1.5707964f && h < 4.712389f) h = pymod(h + pi, two_pi);   // the RoI points the other way
    if (h > pi) h = h - two_pi;
    h = fminf(fmaxf(h, -1.5707964f), 1.5707964f);
    float *enc = a.gt_enc + t * 8;
    enc[0] = x;
    enc[1] = y;
    for (int e = 2; e < 6; ++e) enc[e] = d[e];
    enc[6] = h;
    enc[7] = src[7];
    a.reg_valid[t] = iou > a.reg_fg ? 1 : 0;
    if (a.soft) {   // proposal_target_layer.py:40-47
        float v = iou > a.cls_fg ? 1.f : 0.f;
        if (!(iou > a.cls_fg) && !(iou < a.cls_bg)) v = (iou - a.cls_bg) / a.cls_span;
        ((float *)a.cls_labels)[t] = v;
    } else {        // :34-38
        int64_t v = iou > a.cls_fg ? 1 : 0;
        if (iou > a.cls_bg && iou < a.cls_fg) v = -1;
        ((int64_t *)a.cls_labels)[t] = v;
    }
}

// ---- refine -------------------------------------------------------------------------------------------------------------------------------
// RoI t of the flat [n] lists: the one statement of the arithmetic, shared by the two kernels below
__device__ __forceinline__ void refine_row(const float *__restrict__ rois, const float *__restrict__ roi_scores,
                                           const int64_t *__restrict__ roi_labels, const float *__restrict__ cls, const float *__restrict__ reg,
                                           int64_t t, float *__restrict__ boxes, float *__restrict__ scores, int64_t *__restrict__ labels) {
    const float *roi = rois + t * 7, *res = reg + t * 7;
    float v[7];
    for (int e = 0; e < 3; ++e) v[e] = res[e] + 0.f;   // roi_head_template.py:166-171: the RoI's centre is zeroed before the sum
    for (int e = 3; e < 7; ++e) v[e] = res[e] + roi[e];
    const float ca = cosf(roi[6]), sa = sinf(roi[6]);
    const float x = v[0] * ca + v[1] * sa, y = -v[0] * sa + v[1] * ca;
    float *o = boxes + t * 7;
    o[0] = x + roi[0];
    o[1] = y + roi[1];
    o[2] = v[2] + roi[2];
    for (int e = 3; e < 7; ++e) o[e] = v[e];
    scores[t] = sqrtf(1.f / (1.f + expf(-cls[t])) * roi_scores[t]);
    labels[t] = roi_labels[t] - 1;
}

__global__ __launch_bounds__(256) void roi_refine_kernel(const float *__restrict__ rois, const float *__restrict__ roi_scores,
                                                         const int64_t *__restrict__ roi_labels, const float *__restrict__ cls,
                                                         const float *__restrict__ reg, int64_t n, float *__restrict__ boxes,
                                                         float *__restrict__ scores, int64_t *__restrict__ labels) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    refine_row(rois, roi_scores, roi_labels, cls, reg, t, boxes, scores, labels);
}

// [B][cap] with counts [B] on the device: the rows at and behind counts[b] are written as zeros with label -1 and their inputs are not
// read, so every output element is a function of the rows below the counts alone (the MLP's values for the padding never arrive)
__global__ __launch_bounds__(256) void roi_refine_static_kernel(const float *__restrict__ rois, const float *__restrict__ roi_scores,
                                                                const int64_t *__restrict__ roi_labels, const float *__restrict__ cls,
                                                                const float *__restrict__ reg, const int32_t *__restrict__ counts, int cap,
                                                                float *__restrict__ boxes, float *__restrict__ scores,
                                                                int64_t *__restrict__ labels) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const int64_t t = (int64_t)b * cap + i;
    if (i < counts[b]) {
        refine_row(rois, roi_scores, roi_labels, cls, reg, t, boxes, scores, labels);
        return;
    }
    for (int e = 0; e < 7; ++e) boxes[t * 7 + e] = 0.f;
    scores[t] = 0.f;
    labels[t] = -1;
}

}  // namespace s2d

using namespace s2d;

extern "C" int s2d_roi_pack(const float *boxes, const float *scores, const int64_t *labels, int box_dim, const int32_t *offsets, int batch, int cap,
                            float *rois, float *roi_scores, int64_t *roi_labels, s2d_stream_t stream) {
    S2D_CHECK_ARG(batch >= 0 && batch <= ROI_MAX_BATCH && cap >= 0, "roi_pack: batch %d (0..%d), cap %d", batch, ROI_MAX_BATCH, cap);
    S2D_CHECK_ARG(box_dim >= 7, "roi_pack: box_dim %d (>= 7, heading last)", box_dim);
    if ((int64_t)batch * cap == 0) return S2D_OK;
    S2D_CHECK_ARG(offsets && rois && roi_scores && roi_labels, "roi_pack: null argument");
    PackOffsets off;
    for (int b = 0; b <= batch; ++b) {
        S2D_CHECK_ARG(offsets[b] >= 0 && (b == 0 || offsets[b] >= offsets[b - 1]), "roi_pack: offsets must not decrease (entry %d is %d)", b, offsets[b]);
        off.at[b] = offsets[b];
    }
    for (int b = batch + 1; b <= ROI_MAX_BATCH; ++b) off.at[b] = offsets[batch];
    S2D_CHECK_ARG(offsets[batch] == 0 || (boxes && scores && labels), "roi_pack: null box list");
    hipLaunchKernelGGL(roi_pack_kernel, dim3((unsigned)ceil_div(cap, 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, boxes, scores, labels,
                       box_dim, off, cap, rois, roi_scores, roi_labels);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_roi_pack_static(const float *boxes, const float *scores, const int64_t *labels, const int32_t *counts, int batch, int det_cap,
                                   int cap, float *rois, float *roi_scores, int64_t *roi_labels, int32_t *row, int32_t *out_counts,
                                   s2d_stream_t stream) {
    S2D_CHECK_ARG(batch >= 1 && batch <= ROI_MAX_BATCH, "roi_pack_static: batch %d (1..%d)", batch, ROI_MAX_BATCH);
    S2D_CHECK_ARG(det_cap >= 1 && cap >= 1, "roi_pack_static: det_cap %d, cap %d (>= 1 each)", det_cap, cap);
    S2D_CHECK_ARG((int64_t)batch * det_cap < (1ll << 31), "roi_pack_static: %lld detection rows (int32 row table)", (long long)batch * det_cap);
    S2D_CHECK_ARG(boxes && scores && labels && counts, "roi_pack_static: null boxes, scores, labels or counts");
    S2D_CHECK_ARG(rois && roi_scores && roi_labels && row && out_counts, "roi_pack_static: null output");
    hipLaunchKernelGGL(roi_pack_static_kernel, dim3((unsigned)ceil_div(cap, 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, boxes, scores,
                       labels, counts, det_cap, cap, rois, roi_scores, roi_labels, row, out_counts);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_roi_bev_features(const void *map, int map_dtype, int batch, int channels, int h, int w, int64_t stride_b, int64_t stride_c,
                                    int64_t stride_h, int64_t stride_w, const float *boxes, int64_t total, int box_dim, const int32_t *row, int cap,
                                    int num_point, float pc_x, float pc_y, float voxel_x, float voxel_y, float out_stride, float *feats,
                                    s2d_stream_t stream) {
    S2D_CHECK_ARG(map_dtype == 0 || map_dtype == 1, "roi_bev_features: map dtype %d (0 fp32, 1 bf16)", map_dtype);
    S2D_CHECK_ARG(num_point == 1 || num_point == 5, "roi_bev_features: num_point %d (1 or 5 supported)", num_point);
    S2D_CHECK_ARG(batch >= 0 && cap >= 0 && total >= 0, "roi_bev_features: negative size (batch %d, cap %d, total %lld)", batch, cap, (long long)total);
    S2D_CHECK_ARG(channels >= 1 && h >= 1 && w >= 1, "roi_bev_features: empty map (channels %d, h %d, w %d)", channels, h, w);
    S2D_CHECK_ARG(stride_b >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, "roi_bev_features: negative stride");
    S2D_CHECK_ARG(total < (1ll << 31), "roi_bev_features: %lld boxes (int32 row table)", (long long)total);
    S2D_CHECK_ARG(box_dim >= 7, "roi_bev_features: box_dim %d (>= 7, heading last)", box_dim);
    const int64_t pairs = (int64_t)batch * cap * num_point;
    S2D_CHECK_ARG(ceil_div(pairs, 4) < (1ll << 31), "roi_bev_features: %lld sample points", (long long)pairs);
    if (pairs == 0) return S2D_OK;
    S2D_CHECK_ARG(map && row && feats, "roi_bev_features: null argument");
    S2D_CHECK_ARG(total == 0 || boxes, "roi_bev_features: null box list");
    const FeatArgs a{map,   channels, h,   w,         stride_b, stride_c, stride_h, stride_w, boxes,   total,   box_dim,
                     row,   cap,      num_point, pairs, pc_x,     pc_y,     voxel_x,  voxel_y,  out_stride, feats};
    const dim3 grid((unsigned)ceil_div(pairs, 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    // the 16-byte forms need contiguous channels and every tap row and output row on a 16-byte boundary
    auto rows_aligned = [&](int vec) {
        return stride_c == 1 && channels % vec == 0 && channels % 4 == 0 && stride_b % vec == 0 && stride_h % vec == 0 && stride_w % vec == 0 &&
               (uintptr_t)map % 16 == 0 && (uintptr_t)feats % 16 == 0;
    };
    if (map_dtype == 1) {
        if (rows_aligned(8))
            hipLaunchKernelGGL((roi_bev_features_kernel<unsigned short, 8>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((roi_bev_features_kernel<unsigned short, 1>), grid, block, 0, st, a);
    } else {
        if (rows_aligned(4))
            hipLaunchKernelGGL((roi_bev_features_kernel<float, 4>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((roi_bev_features_kernel<float, 1>), grid, block, 0, st, a);
    }
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_roi_match_gt(const float *rois, const int64_t *roi_labels, int batch, int cap, const float *gt, int num_gt, int gt_dim, int by_class,
                                float *max_iou, int64_t *assignment, int32_t *gt_count, s2d_stream_t stream) {
    S2D_CHECK_ARG(batch >= 0 && batch <= 65535 && cap >= 0, "roi_match_gt: batch %d (0..65535), cap %d", batch, cap);
    S2D_CHECK_ARG(num_gt >= 1 && num_gt <= ROI_MAX_GT, "roi_match_gt: %d ground-truth rows per sample (1..%d supported)", num_gt, ROI_MAX_GT);
    S2D_CHECK_ARG(gt_dim >= 8, "roi_match_gt: gt_dim %d (>= 8: seven box columns, the class last)", gt_dim);
    if (batch == 0) return S2D_OK;
    S2D_CHECK_ARG(gt && gt_count, "roi_match_gt: null ground truth or count");
    S2D_CHECK_ARG(cap == 0 || (rois && roi_labels && max_iou && assignment), "roi_match_gt: null argument");
    // (cap == 0 still runs one block per sample: the counts are an output)
    hipLaunchKernelGGL(roi_match_gt_kernel, dim3((unsigned)(cap ? ceil_div(cap, MATCH_ROIS_PER_BLOCK) : 1), (unsigned)batch), dim3(256), 0,
                       (hipStream_t)stream, rois, roi_labels, cap, gt, num_gt, gt_dim, by_class != 0, max_iou, assignment, gt_count);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_roi_targets(const int32_t *idx, int batch, int per, int cap, int roi_dim, const float *rois, const int64_t *roi_labels,
                               const float *roi_scores, const float *max_iou, const int64_t *assignment, const float *gt, int num_gt, int gt_dim,
                               double reg_fg_thresh, double cls_fg_thresh, double cls_bg_thresh, int cls_score_type, float *out_rois, int64_t *out_labels,
                               float *out_scores, float *out_iou, float *gt_of_rois_src, float *gt_of_rois, int64_t *reg_valid_mask,
                               void *rcnn_cls_labels, s2d_stream_t stream) {
    S2D_CHECK_ARG(roi_dim == 7, "roi_targets: roi_dim %d (code size 7 only)", roi_dim);
    S2D_CHECK_ARG(batch >= 0 && per >= 0, "roi_targets: negative size (batch %d, per %d)", batch, per);
    S2D_CHECK_ARG(cap >= 1 && num_gt >= 1 && gt_dim >= 8, "roi_targets: cap %d, %d ground-truth rows, gt_dim %d (>= 1, >= 1, >= 8)", cap, num_gt, gt_dim);
    S2D_CHECK_ARG(cls_score_type == 0 || cls_score_type == 1, "roi_targets: cls_score_type %d (0 cls, 1 roi_iou)", cls_score_type);
    const int64_t n = (int64_t)batch * per;
    if (n == 0) return S2D_OK;
    S2D_CHECK_ARG(idx && rois && roi_labels && roi_scores && max_iou && assignment && gt, "roi_targets: null input");
    S2D_CHECK_ARG(out_rois && out_labels && out_scores && out_iou && gt_of_rois_src && gt_of_rois && reg_valid_mask && rcnn_cls_labels,
                  "roi_targets: null output");
    TargetArgs a;
    a.idx = idx, a.n = n, a.per = per, a.cap = cap, a.num_gt = num_gt, a.gt_dim = gt_dim;
    a.rois = rois, a.roi_scores = roi_scores, a.max_iou = max_iou, a.gt = gt, a.roi_labels = roi_labels, a.assignment = assignment;
    // python scalars meet fp32 tensors as their fp32 rounding; the span is formed in double first, as `(fg - bg)` is
    a.reg_fg = (float)reg_fg_thresh, a.cls_fg = (float)cls_fg_thresh, a.cls_bg = (float)cls_bg_thresh;
    a.cls_span = (float)(cls_fg_thresh - cls_bg_thresh);
    a.soft = cls_score_type;
    a.out_rois = out_rois, a.out_scores = out_scores, a.out_iou = out_iou, a.gt_src = gt_of_rois_src, a.gt_enc = gt_of_rois;
    a.out_labels = out_labels, a.reg_valid = reg_valid_mask, a.cls_labels = rcnn_cls_labels;
    hipLaunchKernelGGL(roi_targets_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, a);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_roi_refine(const float *rois, const float *roi_scores, const int64_t *roi_labels, const float *rcnn_cls, const float *rcnn_reg,
                              int64_t n, float *boxes, float *scores, int64_t *labels, s2d_stream_t stream) {
    S2D_CHECK_ARG(n >= 0 && ceil_div(n, 256) < (1ll << 31), "roi_refine: %lld RoIs", (long long)n);
    if (n == 0) return S2D_OK;
    S2D_CHECK_ARG(rois && roi_scores && roi_labels && rcnn_cls && rcnn_reg, "roi_refine: null input");
    S2D_CHECK_ARG(boxes && scores && labels, "roi_refine: null output");
    hipLaunchKernelGGL(roi_refine_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, rois, roi_scores, roi_labels, rcnn_cls,
                       rcnn_reg, n, boxes, scores, labels);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_roi_refine_static(const float *rois, const float *roi_scores, const int64_t *roi_labels, const float *rcnn_cls,
                                     const float *rcnn_reg, const int32_t *counts, int batch, int cap, float *boxes, float *scores,
                                     int64_t *labels, s2d_stream_t stream) {
    S2D_CHECK_ARG(batch >= 1 && batch <= 65535 && cap >= 1, "roi_refine_static: batch %d (1..65535), cap %d (>= 1)", batch, cap);
    S2D_CHECK_ARG(rois && roi_scores && roi_labels && rcnn_cls && rcnn_reg && counts, "roi_refine_static: null input");
    S2D_CHECK_ARG(boxes && scores && labels, "roi_refine_static: null output");
    hipLaunchKernelGGL(roi_refine_static_kernel, dim3((unsigned)ceil_div(cap, 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, rois,
                       roi_scores, roi_labels, rcnn_cls, rcnn_reg, counts, cap, boxes, scores, labels);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
