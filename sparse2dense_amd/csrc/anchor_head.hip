// SECOND anchor head on the device (Waymo configuration: one task, `ground_box3d_coder` 7-wide, nearest-IoU similarity, no sampling,
// NormByNumPositives, sigmoid focal + codewise smooth-L1 + softmax direction loss, sin-difference angle coding):
//   (a) AssignTarget / TargetAssigner.assign_v2 / create_target_np
//       (det3d/datasets/pipelines/preprocess.py:726-830, det3d/core/anchor/target_assigner.py:68-137,
//        det3d/core/anchor/target_ops.py:29-223) with rbbox2d_to_near_bbox, iou_jit(eps=0), limit_period and second_box_encode of
//        det3d/core/bbox/box_np_ops.py:131-143,360-361,497-535,1002-1063 - per-frame numpy / numba on the host in the reference;
//   (b,c) prepare_loss_weights + create_loss + add_sin_difference + get_direction_target + the reductions of MultiGroupHead.loss
//       (det3d/models/bbox_heads/mg_head.py:29-63,147-188,535-667; det3d/models/losses/losses.py:147-222,293-359,431-469) - several dozen
//       elementwise launches over [B, 212 064, .] tensors in the reference, one pass + a finalize here, one pass backward;
//   (d) the per-anchor part of MultiGroupHead.predict (mg_head.py:737-765,838-849,995-1001 with second_box_decode of
//       det3d/core/bbox/box_torch_ops.py:87-150).
// Anchor a of a frame sits in slot a % (classes * rotations) of its cell; slots [c * rotations, (c + 1) * rotations) belong to class c
// (generate_anchors concatenates the classes along the slot axis, target_assigner.py:139-158).
// Sums are per-block slabs folded in a fixed order (no float atomics): every result is bitwise reproducible run to run.
#include "anchor_decode.h"

namespace s2d {

constexpr int AH_MAX_BOXES = 500;
constexpr int AH_MAX_CLASSES = 8;
constexpr int AH_LOSS_BLOCKS = 104;   // per frame; 256 threads each: ~8 anchors per thread at 212 064 anchors
constexpr int AH_SUMS = 12;           // cls channel 0 | cls channels 1.. | loc[7] | dir | positives | negatives

struct AhAssign {
    float matched[AH_MAX_CLASSES], unmatched[AH_MAX_CLASSES];
    int classes, rotations, max_boxes;
    int64_t anchors;
};

struct AhLoss {
    float pos_w, neg_w, alpha, sigma, loc_w, cls_w, dir_w, dir_offset;
    int classes, frames;
    int64_t anchors;
};

__device__ __forceinline__ float ah_block_sum(float v, float *sh) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wid] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ float ah_limit_period(float v, float period) { return v - floorf(v / period + 0.5f) * period; }

// rbbox2d_to_near_bbox on (x, y, w, l, r): the axis-aligned box of the nearest standing / lying rectangle (fp32, as numpy on fp32 arrays)
__device__ __forceinline__ void ah_near_bbox(float x, float y, float w, float l, float r, float out[4]) {
    const float lim = fabsf(ah_limit_period(r, (float)3.141592653589793));
    const bool lying = lim > (float)(3.141592653589793 / 4);
    const float dx = lying ? l : w, dy = lying ? w : l;
    out[0] = x - dx / 2.f;
    out[1] = y - dy / 2.f;
    out[2] = x + dx / 2.f;
    out[3] = y + dy / 2.f;
}

// iou_jit(eps = 0) of two axis-aligned boxes: float64 intermediates, one rounding to fp32 (so that `==` between two entries of the
// overlap matrix is exact); the early-outs define which entries stay exactly 0
__device__ __forceinline__ float ah_iou(const float a[4], float q0, float q1, float q2, float q3) {
    const double iw = (double)fminf(a[2], q2) - (double)fmaxf(a[0], q0);
    if (!(iw > 0)) return 0.f;
    const double ih = (double)fminf(a[3], q3) - (double)fmaxf(a[1], q1);
    if (!(ih > 0)) return 0.f;
    const double box_area = ((double)q2 - (double)q0) * ((double)q3 - (double)q1);
    const double ua = ((double)a[2] - (double)a[0]) * ((double)a[3] - (double)a[1]) + box_area - iw * ih;
    return (float)(iw * ih / ua);
}

// the frame's boxes -> LDS: near bbox (with the yaw limited to [-pi, pi) first, preprocess.py:759-763) and class
__device__ __forceinline__ void ah_stage_boxes(const float *__restrict__ boxes, const int32_t *__restrict__ classes, int max_boxes, float (*q)[AH_MAX_BOXES],
                                               int *cls) {
    for (int k = threadIdx.x; k < max_boxes; k += blockDim.x) {
        const float *bx = boxes + (int64_t)k * 7;
        float nb[4];
        ah_near_bbox(bx[0], bx[1], bx[3], bx[4], ah_limit_period(bx[6], (float)(3.141592653589793 * 2)), nb);
        q[0][k] = nb[0]; q[1][k] = nb[1]; q[2][k] = nb[2]; q[3][k] = nb[3];
        cls[k] = classes[k];
    }
}

// pass 1: per box the maximum overlap over the anchors of its class (bit pattern of a non-negative float: ordered like the int)
__global__ __launch_bounds__(256) void anchor_assign_colmax_kernel(const float *__restrict__ gt_boxes, const int32_t *__restrict__ gt_classes,
                                                                   const float *__restrict__ anchors, AhAssign g, int *__restrict__ colmax) {
    __shared__ float q[4][AH_MAX_BOXES];
    __shared__ int cls[AH_MAX_BOXES], cmax[AH_MAX_BOXES];
    const int b = blockIdx.y, K = g.max_boxes;
    ah_stage_boxes(gt_boxes + (int64_t)b * K * 7, gt_classes + (int64_t)b * K, K, q, cls);
    for (int k = threadIdx.x; k < K; k += 256) cmax[k] = 0;
    __syncthreads();
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a < g.anchors) {
        const float *an = anchors + a * 7;
        const int want = (int)(a % (g.classes * g.rotations)) / g.rotations + 1;
        float nb[4];
        ah_near_bbox(an[0], an[1], an[3], an[4], an[6], nb);
        for (int k = 0; k < K; ++k) {
            if (cls[k] != want) continue;
            const float iou = ah_iou(nb, q[0][k], q[1][k], q[2][k], q[3][k]);
            if (iou > 0.f) atomicMax(&cmax[k], __float_as_int(iou));
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256)
        if (cmax[k] > 0) atomicMax(colmax + (int64_t)b * K + k, cmax[k]);
}

// pass 2: row maximum / first-index argmax, the tie test against the column maxima, label, encoding, weight
__global__ __launch_bounds__(256) void anchor_assign_label_kernel(const float *__restrict__ gt_boxes, const int32_t *__restrict__ gt_classes,
                                                                  const float *__restrict__ anchors, AhAssign g, const int *__restrict__ colmax,
                                                                  int32_t *__restrict__ labels, float *__restrict__ reg_targets,
                                                                  float *__restrict__ reg_weights) {
    __shared__ float q[4][AH_MAX_BOXES];
    __shared__ int cls[AH_MAX_BOXES], cmax[AH_MAX_BOXES];
    const int b = blockIdx.y, K = g.max_boxes;
    ah_stage_boxes(gt_boxes + (int64_t)b * K * 7, gt_classes + (int64_t)b * K, K, q, cls);
    for (int k = threadIdx.x; k < K; k += 256) cmax[k] = colmax[(int64_t)b * K + k];
    __syncthreads();
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= g.anchors) return;
    const float *an = anchors + a * 7;
    const int c = (int)(a % (g.classes * g.rotations)) / g.rotations;
    float nb[4];
    ah_near_bbox(an[0], an[1], an[3], an[4], an[6], nb);
    float best = 0.f;
    int arg = -1;
    bool forced = false;
    for (int k = 0; k < K; ++k) {
        if (cls[k] != c + 1) continue;
        const float iou = ah_iou(nb, q[0][k], q[1][k], q[2][k], q[3][k]);
        if (arg < 0 || iou > best) {
            best = iou;
            arg = k;
        }
        // a box whose maximum is 0 never forces a match; a forced anchor goes to ITS OWN argmax box (target_ops.py:111-127)
        forced |= iou > 0.f && __float_as_int(iou) == cmax[k];
    }
    int label = 0;
    float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (arg >= 0) {
        if (forced || best >= g.matched[c])
            label = c + 1;
        else if (!(best < g.unmatched[c]))
            label = -1;
    }
    if (label > 0) {   // second_box_encode(gt[argmax], anchor), fp32
        const float *bx = gt_boxes + ((int64_t)b * K + arg) * 7;
        const float diagonal = sqrtf(an[4] * an[4] + an[3] * an[3]);
        t[0] = (bx[0] - an[0]) / diagonal;
        t[1] = (bx[1] - an[1]) / diagonal;
        t[2] = (bx[2] - an[2]) / an[5];
        t[3] = logf(bx[3] / an[3]);
        t[4] = logf(bx[4] / an[4]);
        t[5] = logf(bx[5] / an[5]);
        t[6] = ah_limit_period(bx[6], (float)(3.141592653589793 * 2)) - an[6];
    }
    const int64_t at = (int64_t)b * g.anchors + a;
    labels[at] = label;
    reg_weights[at] = label > 0 ? 1.f : 0.f;
#pragma unroll
    for (int e = 0; e < 7; ++e) reg_targets[at * 7 + e] = t[e];
}

// ---- loss -----------------------------------------------------------------------------------------------------------------------------
// one class logit of SigmoidFocalLoss(gamma = 2): value and derivative, before the anchor's weight
__device__ __forceinline__ void ah_focal(float x, bool target, float alpha, float &value, float &grad) {
    const float e = expf(-fabsf(x));
    const float soft = log1pf(e);                                  // log1p(exp(-|x|))
    const float p = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);     // sigmoid(x)
    if (target) {
        const float ce = fmaxf(x, 0.f) - x + soft, om = 1.f - p;
        value = om * om * alpha * ce;
        grad = -alpha * om * om * (om + 2.f * p * ce);
    } else {
        const float ce = fmaxf(x, 0.f) + soft, w = 1.f - alpha;
        value = p * p * w * ce;
        grad = w * p * p * (2.f * (1.f - p) * ce + p);
    }
}

__device__ __forceinline__ bool ah_dir_target(float reg_rot, float anchor_rot, float offset) {
    return ah_limit_period(reg_rot + anchor_rot - offset, (float)(3.141592653589793 * 2)) > 0.f;
}

__global__ __launch_bounds__(256) void anchor_loss_fwd_kernel(const float *__restrict__ box_preds, const float *__restrict__ cls_preds,
                                                              const float *__restrict__ dir_preds, const int32_t *__restrict__ labels,
                                                              const float *__restrict__ reg_targets, const float *__restrict__ anchors, AhLoss g,
                                                              float *__restrict__ partial) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    float s[AH_SUMS];
#pragma unroll
    for (int i = 0; i < AH_SUMS; ++i) s[i] = 0.f;
    const float cond = 1.f / (g.sigma * g.sigma);
    for (int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x; a < g.anchors; a += (int64_t)gridDim.x * 256) {
        const int64_t at = (int64_t)b * g.anchors + a;
        const int label = labels[at];
        if (label < 0) continue;   // ignored: every weight is 0
        const float w = label > 0 ? g.pos_w : g.neg_w;
        for (int j = 0; j < g.classes; ++j) {
            float v, dv;
            ah_focal(cls_preds[at * g.classes + j], label == j + 1, g.alpha, v, dv);
            s[j == 0 ? 0 : 1] += v * w;
        }
        if (label > 0) {
            const float *p = box_preds + at * 7, *t = reg_targets + at * 7;
#pragma unroll
            for (int e = 0; e < 7; ++e) {
                const float d = e < 6 ? p[e] - t[e] : sinf(p[6]) * cosf(t[6]) - cosf(p[6]) * sinf(t[6]);
                const float ad = fabsf(d);
                s[2 + e] += ad <= cond ? 0.5f * (ad * g.sigma) * (ad * g.sigma) : ad - 0.5f / (g.sigma * g.sigma);
            }
            const float d0 = dir_preds[at * 2], d1 = dir_preds[at * 2 + 1], m = fmaxf(d0, d1);
            const float lse = m + logf(expf(d0 - m) + expf(d1 - m));
            s[9] += lse - (ah_dir_target(t[6], anchors[a * 7 + 6], g.dir_offset) ? d1 : d0);
            s[10] += 1.f;
        } else {
            s[11] += 1.f;
        }
    }
    float *out = partial + ((int64_t)b * gridDim.x + blockIdx.x) * AH_SUMS;
#pragma unroll
    for (int i = 0; i < AH_SUMS; ++i) {
        const float v = ah_block_sum(s[i], sh);
        if (threadIdx.x == 0) out[i] = v;
    }
}

// res: loss | cls_pos_loss | cls_neg_loss | dir_loss_reduced | cls_loss_reduced | loc_loss_reduced | loc_loss_elem[7] | num_pos | num_neg
// norm[b] = 1 / clamp(positives of frame b, 1)
__global__ __launch_bounds__(256) void anchor_loss_finalize_kernel(const float *__restrict__ partial, int blocks, AhLoss g, float *__restrict__ folded,
                                                                   float *__restrict__ res, float *__restrict__ norm) {
    for (int i = threadIdx.x; i < g.frames * AH_SUMS; i += 256) {
        const int b = i / AH_SUMS, e = i - b * AH_SUMS;
        float v = 0.f;
        for (int k = 0; k < blocks; ++k) v += partial[((int64_t)b * blocks + k) * AH_SUMS + e];
        folded[i] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float cls0 = 0.f, cls1 = 0.f, dir = 0.f, loc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < g.frames; ++b) {
        const float *f = folded + b * AH_SUMS;
        const float n = 1.f / fmaxf(f[10], 1.f);
        norm[b] = n;
        cls0 += f[0] * n;
        cls1 += f[1] * n;
        for (int e = 0; e < 7; ++e) loc[e] += f[2 + e] * n;
        dir += f[9] * n;
    }
    const float inv_b = 1.f / (float)g.frames;
    float loc_sum = 0.f;
    for (int e = 0; e < 7; ++e) {
        loc_sum += loc[e];
        res[6 + e] = loc[e] * inv_b;
    }
    const float loc_red = loc_sum * inv_b * g.loc_w, cls_red = (cls0 + cls1) * inv_b * g.cls_w, dir_red = dir * inv_b;
    res[0] = loc_red + cls_red + dir_red * g.dir_w;
    res[1] = cls1 * inv_b / g.pos_w;
    res[2] = cls0 * inv_b / g.neg_w;
    res[3] = dir_red;
    res[4] = cls_red;
    res[5] = loc_red;
    res[13] = folded[10];
    res[14] = folded[11];
}

__global__ __launch_bounds__(256) void anchor_loss_bwd_kernel(const float *__restrict__ box_preds, const float *__restrict__ cls_preds,
                                                              const float *__restrict__ dir_preds, const int32_t *__restrict__ labels,
                                                              const float *__restrict__ reg_targets, const float *__restrict__ anchors, AhLoss g,
                                                              const float *__restrict__ norm, const float *__restrict__ go, float *__restrict__ dbox,
                                                              float *__restrict__ dcls, float *__restrict__ ddir) {
    const int b = blockIdx.y;
    const float scale = go[0] * norm[b] / (float)g.frames;
    const float cond = 1.f / (g.sigma * g.sigma);
    for (int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x; a < g.anchors; a += (int64_t)gridDim.x * 256) {
        const int64_t at = (int64_t)b * g.anchors + a;
        const int label = labels[at];
        const float w = label > 0 ? g.pos_w : (label == 0 ? g.neg_w : 0.f);
        for (int j = 0; j < g.classes; ++j) {
            float v = 0.f, dv = 0.f;
            if (label >= 0) ah_focal(cls_preds[at * g.classes + j], label == j + 1, g.alpha, v, dv);
            dcls[at * g.classes + j] = label >= 0 ? dv * w * scale * g.cls_w : 0.f;
        }
        float db[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dd0 = 0.f, dd1 = 0.f;
        if (label > 0) {
            const float *p = box_preds + at * 7, *t = reg_targets + at * 7;
            const float sp = sinf(p[6]), cp = cosf(p[6]), st = sinf(t[6]), ct = cosf(t[6]);
#pragma unroll
            for (int e = 0; e < 7; ++e) {
                const float d = e < 6 ? p[e] - t[e] : sp * ct - cp * st;
                const float slope = fabsf(d) <= cond ? g.sigma * g.sigma * d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
                db[e] = slope * (e < 6 ? 1.f : cp * ct + sp * st) * scale * g.loc_w;
            }
            const float d0 = dir_preds[at * 2], d1 = dir_preds[at * 2 + 1], m = fmaxf(d0, d1);
            const float e0 = expf(d0 - m), e1 = expf(d1 - m), inv = 1.f / (e0 + e1);
            const bool tgt = ah_dir_target(t[6], anchors[a * 7 + 6], g.dir_offset);
            dd0 = (e0 * inv - (tgt ? 0.f : 1.f)) * scale * g.dir_w;
            dd1 = (e1 * inv - (tgt ? 1.f : 0.f)) * scale * g.dir_w;
        }
#pragma unroll
        for (int e = 0; e < 7; ++e) dbox[at * 7 + e] = db[e];
        ddir[at * 2] = dd0;
        ddir[at * 2 + 1] = dd1;
    }
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void anchor_decode_kernel(const float *__restrict__ box_preds, const float *__restrict__ cls_preds,
                                                            const float *__restrict__ dir_preds, const float *__restrict__ anchors, int64_t total,
                                                            int64_t num_anchors, int classes, float score_threshold, float *__restrict__ boxes,
                                                            float *__restrict__ scores, int32_t *__restrict__ labels,
                                                            int32_t *__restrict__ dir_labels, uint8_t *__restrict__ keep) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= total) return;
    const float *an = anchors + (at % num_anchors) * 7, *t = box_preds + at * 7;
    int arg;
    const float best = anchor_class_max(cls_preds + at * classes, classes, arg);
    anchor_box_decode(t, an, boxes + at * 7);
    scores[at] = best;
    labels[at] = arg;
    dir_labels[at] = dir_preds ? (dir_preds[at * 2 + 1] > dir_preds[at * 2] ? 1 : 0) : 0;
    keep[at] = best >= score_threshold ? 1 : 0;
}

static int ah_loss_args(const float *params, int frames, int64_t num_anchors, int num_classes, AhLoss *g, const char *who) {
    S2D_CHECK_ARG(params, "%s: null params", who);
    S2D_CHECK_ARG(frames > 0 && frames <= 65535 && num_anchors > 0 && num_classes > 0 && num_classes <= AH_MAX_CLASSES,
                  "%s: bad sizes (frames %d, num_anchors %lld, num_classes %d)", who, frames, (long long)num_anchors, num_classes);
    S2D_CHECK_ARG(params[3] == 2.f, "%s: gamma %g is not supported (SigmoidFocalLoss gamma must be 2)", who, (double)params[3]);
    S2D_CHECK_ARG(params[4] > 0.f && params[0] > 0.f && params[1] > 0.f, "%s: sigma and the class weights must be positive", who);
    *g = AhLoss{params[0], params[1], params[2], params[4], params[5], params[6], params[7], params[8], num_classes, frames, num_anchors};
    return S2D_OK;
}

}  // namespace s2d

using namespace s2d;

extern "C" size_t s2d_anchor_assign_workspace_bytes(int frames, int max_boxes) {
    if (frames <= 0 || max_boxes <= 0) return 0;
    return align_up((size_t)frames * max_boxes * sizeof(int), 256);
}

extern "C" int s2d_anchor_assign(const float *gt_boxes, const int32_t *gt_classes, int frames, int max_boxes, const float *anchors,
                                 int64_t num_anchors, int num_classes, int rotations, const float *matched_thresholds,
                                 const float *unmatched_thresholds, int32_t *labels, float *reg_targets, float *reg_weights, void *ws,
                                 size_t ws_bytes, s2d_stream_t stream) {
    S2D_CHECK_ARG(frames > 0 && frames <= 65535, "anchor_assign: bad frames %d", frames);
    S2D_CHECK_ARG(max_boxes > 0 && max_boxes <= AH_MAX_BOXES, "anchor_assign: max_boxes %d outside 1..%d", max_boxes, AH_MAX_BOXES);
    S2D_CHECK_ARG(num_classes > 0 && num_classes <= AH_MAX_CLASSES && rotations > 0, "anchor_assign: bad num_classes %d / rotations %d",
                  num_classes, rotations);
    S2D_CHECK_ARG(num_anchors > 0 && num_anchors % (num_classes * rotations) == 0,
                  "anchor_assign: num_anchors %lld is not a multiple of the %d slots per cell", (long long)num_anchors, num_classes * rotations);
    S2D_CHECK_ARG(gt_boxes && gt_classes && anchors && matched_thresholds && unmatched_thresholds, "anchor_assign: null input");
    S2D_CHECK_ARG(labels && reg_targets && reg_weights, "anchor_assign: null output");
    if (!ws || ws_bytes < s2d_anchor_assign_workspace_bytes(frames, max_boxes)) {
        set_error("anchor_assign: workspace too small");
        return S2D_ERR_WORKSPACE;
    }
    AhAssign g{};
    for (int c = 0; c < num_classes; ++c) {
        g.matched[c] = matched_thresholds[c];
        g.unmatched[c] = unmatched_thresholds[c];
    }
    g.classes = num_classes;
    g.rotations = rotations;
    g.max_boxes = max_boxes;
    g.anchors = num_anchors;
    hipStream_t st = (hipStream_t)stream;
    int *colmax = (int *)ws;
    if (int rc = zero_async(colmax, (size_t)frames * max_boxes * sizeof(int), st)) return rc;   // (a kernel, not a memset node)
    const dim3 grid((unsigned)ceil_div(num_anchors, 256), (unsigned)frames);
    hipLaunchKernelGGL(anchor_assign_colmax_kernel, grid, dim3(256), 0, st, gt_boxes, gt_classes, anchors, g, colmax);
    hipLaunchKernelGGL(anchor_assign_label_kernel, grid, dim3(256), 0, st, gt_boxes, gt_classes, anchors, g, (const int *)colmax, labels,
                       reg_targets, reg_weights);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" size_t s2d_anchor_loss_workspace_bytes(int frames) {
    if (frames <= 0) return 0;
    return align_up((size_t)frames * (AH_LOSS_BLOCKS + 1) * AH_SUMS * sizeof(float), 256);
}

extern "C" int s2d_anchor_loss_fwd(const float *box_preds, const float *cls_preds, const float *dir_cls_preds, const int32_t *labels,
                                   const float *reg_targets, const float *anchors, int frames, int64_t num_anchors, int num_classes,
                                   const float *params, float *res, float *norm, void *ws, size_t ws_bytes, s2d_stream_t stream) {
    AhLoss g;
    if (int rc = ah_loss_args(params, frames, num_anchors, num_classes, &g, "anchor_loss_fwd")) return rc;
    S2D_CHECK_ARG(box_preds && cls_preds && dir_cls_preds && labels && reg_targets && anchors, "anchor_loss_fwd: null input");
    S2D_CHECK_ARG(res && norm, "anchor_loss_fwd: null output");
    if (!ws || ws_bytes < s2d_anchor_loss_workspace_bytes(frames)) {
        set_error("anchor_loss_fwd: workspace too small");
        return S2D_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int blocks = (int)std::min<int64_t>(AH_LOSS_BLOCKS, ceil_div(num_anchors, 256));
    float *partial = (float *)ws, *folded = partial + (size_t)frames * AH_LOSS_BLOCKS * AH_SUMS;
    hipLaunchKernelGGL(anchor_loss_fwd_kernel, dim3(blocks, frames), dim3(256), 0, st, box_preds, cls_preds, dir_cls_preds, labels, reg_targets,
                       anchors, g, partial);
    hipLaunchKernelGGL(anchor_loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const float *)partial, blocks, g, folded, res, norm);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_anchor_loss_bwd(const float *box_preds, const float *cls_preds, const float *dir_cls_preds, const int32_t *labels,
                                   const float *reg_targets, const float *anchors, int frames, int64_t num_anchors, int num_classes,
                                   const float *params, const float *norm, const float *grad_loss, float *d_box_preds, float *d_cls_preds,
                                   float *d_dir_cls_preds, s2d_stream_t stream) {
    AhLoss g;
    if (int rc = ah_loss_args(params, frames, num_anchors, num_classes, &g, "anchor_loss_bwd")) return rc;
    S2D_CHECK_ARG(box_preds && cls_preds && dir_cls_preds && labels && reg_targets && anchors && norm && grad_loss, "anchor_loss_bwd: null input");
    S2D_CHECK_ARG(d_box_preds && d_cls_preds && d_dir_cls_preds, "anchor_loss_bwd: null output");
    const int blocks = (int)std::min<int64_t>(4 * AH_LOSS_BLOCKS, ceil_div(num_anchors, 256));
    hipLaunchKernelGGL(anchor_loss_bwd_kernel, dim3(blocks, frames), dim3(256), 0, (hipStream_t)stream, box_preds, cls_preds, dir_cls_preds, labels,
                       reg_targets, anchors, g, norm, grad_loss, d_box_preds, d_cls_preds, d_dir_cls_preds);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_anchor_decode(const float *box_preds, const float *cls_preds, const float *dir_cls_preds, const float *anchors, int frames,
                                 int64_t num_anchors, int num_classes, float score_threshold, float *boxes, float *scores, int32_t *labels,
                                 int32_t *dir_labels, uint8_t *keep, s2d_stream_t stream) {
    S2D_CHECK_ARG(frames > 0 && num_anchors > 0 && num_classes > 0 && num_classes <= AH_MAX_CLASSES,
                  "anchor_decode: bad sizes (frames %d, num_anchors %lld, num_classes %d)", frames, (long long)num_anchors, num_classes);
    S2D_CHECK_ARG(box_preds && cls_preds && anchors, "anchor_decode: null input");
    S2D_CHECK_ARG(boxes && scores && labels && dir_labels && keep, "anchor_decode: null output");
    const int64_t total = (int64_t)frames * num_anchors;
    hipLaunchKernelGGL(anchor_decode_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, box_preds, cls_preds,
                       dir_cls_preds, anchors, total, num_anchors, num_classes, score_threshold, boxes, scores, labels, dir_labels, keep);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
