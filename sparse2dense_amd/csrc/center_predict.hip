// CenterHead.predict on the device (det3d/models/bbox_heads/center_head.py:293-448 decode, :452-495 post_processing, :499-507 circle NMS):
// every (task, sample) pair - a SEGMENT - of a head goes through four launches instead of a torch chain per segment.
//   center_score_kernel   all tasks, all samples: flip-averaged sigmoid maximum + class, centre, score / range test -> score map (-inf =
//                         dropped), label map, pass count per segment.  The dense [B, H*W, 7|9] box tensor of the chain is never formed.
//   (torch.sort of the score maps, one host read of the counts)
//   center_boxes_kernel   decodes the full box of the n_s best pixels of every segment into one packed list
//   nms_batched_*_kernel  suppression bit matrices of all segments in one launch (rotated IoU or centre distance: the pair tests of
//                         nms.hip, unchanged), then the greedy walk with ONE WORKGROUP PER SEGMENT - the walks are independent
//   predict_static_gather_kernel  (the static path, center_predict.StaticPredictPlan: s2d_segment_topk of segment_topk.hip in place of
//                         the sort, no host read) the kept rows of every sample into outputs of fixed capacity, padding written
// The per-task map pointers and strides travel by value in the kernel arguments (s2d_center_predict_task[8], as s2d_center_task[8] does
// for the loss).  Expression order follows the torch chain (the library is built with -ffp-contract=off): the flip mean is the
// left-to-right sum of the four views times 0.25, x = (col + reg_x) * out_size_factor * voxel_x + pc_x.
// Built without the SLP vectoriser (DESIGN rule 36): predict runs beside the weight-gradient stream in two-stage training.
#include "nms_geom.h"

#include <math.h>

namespace s2d {

constexpr int CP_MAX_TASKS = S2D_CENTER_PREDICT_MAX_TASKS;
enum { M_HM = 0, M_REG, M_HEIGHT, M_DIM, M_VEL, M_ROT };

struct PredictTasks {
    s2d_center_predict_task t[CP_MAX_TASKS];
};

struct PredictGeo {
    int samples, h, w, flip;
    float factor, vx, vy, px, py;
};

// the (up to four) views of output pixel (y, x) of sample b: view 1 mirrored along H, 2 along W, 3 along both (center_head.py:329-333)
struct Views {
    int n;
    int64_t img[4], pix[4];
};

__device__ __forceinline__ Views views_of(const PredictGeo &g, int b, int y, int x) {
    Views v;
    if (!g.flip) {
        v.n = 1;
        v.img[0] = b;
        v.pix[0] = (int64_t)y * g.w + x;
        return v;
    }
    v.n = 4;
    for (int k = 0; k < 4; ++k) {
        const int yy = (k & 1) ? g.h - 1 - y : y, xx = (k & 2) ? g.w - 1 - x : x;
        v.img[k] = (int64_t)b * 4 + k;
        v.pix[k] = (int64_t)yy * g.w + xx;
    }
    return v;
}

__device__ __forceinline__ float map_at(const s2d_center_predict_task &t, int m, int channels, int64_t hw, int64_t img, int c, int64_t pix) {
    return t.map[m][img * channels * hw + c * t.channel_stride[m] + pix * t.pixel_stride[m]];
}

// mean over the views of channel c of map m; bit k of `mirror` replaces view k's value by 1 - value, bit k of `negate` negates it
__device__ __forceinline__ float view_mean(const s2d_center_predict_task &t, int m, int channels, int64_t hw, const Views &v, int c, unsigned negate,
                                           unsigned mirror) {
    float acc = 0.f;
    for (int k = 0; k < v.n; ++k) {
        float a = map_at(t, m, channels, hw, v.img[k], c, v.pix[k]);
        if ((mirror >> k) & 1u) a = 1 - a;
        if ((negate >> k) & 1u) a = a * -1;
        acc = k == 0 ? a : acc + a;
    }
    return v.n == 1 ? acc : acc * 0.25f;
}

__device__ __forceinline__ void centre_of(const s2d_center_predict_task &t, const PredictGeo &g, int64_t hw, const Views &v, int y, int x, float &cx,
                                          float &cy, float &cz) {
    // center_head.py:356-362: the offset inside the cell mirrors with the flip (views 2, 3 along x; views 1, 3 along y)
    const float rx = view_mean(t, M_REG, 2, hw, v, 0, 0u, 0xCu), ry = view_mean(t, M_REG, 2, hw, v, 1, 0u, 0xAu);
    cx = ((float)x + rx) * g.factor * g.vx + g.px;
    cy = ((float)y + ry) * g.factor * g.vy + g.py;
    cz = view_mean(t, M_HEIGHT, 1, hw, v, 0, 0u, 0u);
}

struct ScoreArgs {
    float threshold;
    int has_range;
    float lo[3], hi[3];
};

__global__ __launch_bounds__(256) void center_score_kernel(PredictTasks tasks, PredictGeo g, ScoreArgs a, float *__restrict__ score,
                                                           int32_t *__restrict__ label, int32_t *__restrict__ count) {
    __shared__ int passed;
    const int seg = blockIdx.y, task = seg / g.samples, b = seg % g.samples;
    const s2d_center_predict_task &t = tasks.t[task];
    const int64_t hw = (int64_t)g.h * g.w;
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) passed = 0;
    __syncthreads();
    if (pix < hw) {
        const int y = (int)(pix / g.w), x = (int)(pix % g.w);
        const Views v = views_of(g, b, y, x);
        float best = 0.f;
        int cls = 0;
        bool nan = false;
        for (int c = 0; c < t.classes; ++c) {
            float acc = 0.f;
            for (int k = 0; k < v.n; ++k) {
                const float s = 1.f / (1.f + expf(-map_at(t, M_HM, t.classes, hw, v.img[k], c, v.pix[k])));
                acc = k == 0 ? s : acc + s;
            }
            if (v.n == 4) acc = acc * 0.25f;
            nan |= acc != acc;
            if (c == 0 || acc > best) {   // strict: the lowest class index wins a tie
                best = acc;
                cls = c;
            }
        }
        float cx, cy, cz;
        centre_of(t, g, hw, v, y, x, cx, cy, cz);
        bool keep = !nan && best > a.threshold;   // a NaN maximum compares false in torch as well
        if (a.has_range) keep = keep && cx >= a.lo[0] && cy >= a.lo[1] && cz >= a.lo[2] && cx <= a.hi[0] && cy <= a.hi[1] && cz <= a.hi[2];
        score[(int64_t)seg * hw + pix] = keep ? best : -INFINITY;
        label[(int64_t)seg * hw + pix] = cls;
        if (keep) atomicAdd(&passed, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && passed) atomicAdd(&count[seg], passed);
}

__global__ __launch_bounds__(256) void center_boxes_kernel(PredictTasks tasks, PredictGeo g, const int64_t *__restrict__ order,
                                                           const float *__restrict__ score_sorted, const int32_t *__restrict__ label,
                                                           const int32_t *__restrict__ offsets, const int32_t *__restrict__ counts, int max_count,
                                                           int64_t total, int box_dim, float *__restrict__ boxes, float *__restrict__ scores,
                                                           int64_t *__restrict__ labels) {
    const int seg = blockIdx.y, task = seg / g.samples, b = seg % g.samples;
    const s2d_center_predict_task &t = tasks.t[task];
    const int64_t hw = (int64_t)g.h * g.w;
    const int64_t rank = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = min((int64_t)min(counts[seg], max_count), hw), off = offsets[seg];
    if (rank >= n || off < 0 || off + n > total) return;
    const int64_t pix = order[(int64_t)seg * hw + rank];
    if (pix < 0 || pix >= hw) return;
    const int y = (int)(pix / g.w), x = (int)(pix % g.w);
    const Views v = views_of(g, b, y, x);
    float *bx = boxes + (off + rank) * box_dim;
    centre_of(t, g, hw, v, y, x, bx[0], bx[1], bx[2]);
    for (int c = 0; c < 3; ++c) {   // mean over the views of exp(dim)
        float acc = 0.f;
        for (int k = 0; k < v.n; ++k) {
            const float e = expf(map_at(t, M_DIM, 3, hw, v.img[k], c, v.pix[k]));
            acc = k == 0 ? e : acc + e;
        }
        bx[3 + c] = v.n == 4 ? acc * 0.25f : acc;
    }
    if (t.map[M_VEL]) {   // center_head.py:406-414: view 1 negates vy, view 2 vx, view 3 both
        bx[6] = view_mean(t, M_VEL, 2, hw, v, 0, 0xCu, 0u);
        bx[7] = view_mean(t, M_VEL, 2, hw, v, 1, 0xAu, 0u);
    }
    // center_head.py:364-380: the y-flip negates the cosine (views 1, 3), the x-flip the sine (views 2, 3)
    const float rs = view_mean(t, M_ROT, 2, hw, v, 0, 0xCu, 0u), rc = view_mean(t, M_ROT, 2, hw, v, 1, 0xAu, 0u);
    bx[box_dim - 1] = atan2f(rs, rc);
    scores[off + rank] = score_sorted[(int64_t)seg * hw + rank];
    labels[off + rank] = (int64_t)label[(int64_t)seg * hw + pix] + t.label_base;
}

// ---- batched NMS ----------------------------------------------------------------------------------------------------------------------
// Segment s holds counts[s] (clamped to max_count) rows of the packed list from row offsets[s]; its bit matrix lives at
// mask + offsets[s] * ceil(max_count / 64) with its own row length ceil(n_s / 64).  A segment whose rows do not lie inside [0, total)
// is treated as empty, so a wrong device array cannot lead a kernel outside the workspace.
struct Segment {
    int n, col_blocks;
    int64_t off;
    unsigned long long *mask;
};

__device__ __forceinline__ Segment segment_of(const int32_t *offsets, const int32_t *counts, int seg, int max_count, int64_t total,
                                              unsigned long long *mask) {
    Segment s;
    s.n = min(counts[seg], max_count);
    s.off = offsets[seg];
    if (s.n < 0 || s.off < 0 || s.off + s.n > total) s.n = 0;
    s.col_blocks = (s.n + 63) / 64;
    s.mask = mask + s.off * ((max_count + 63) / 64);
    return s;
}

// CIRCLE: rows are (x, y) at `stride` floats, bit j = (xi - xj)^2 + (yi - yj)^2 <= thresh[seg] (circle_mask_kernel of nms.hip);
// otherwise rows are boxes of `stride` floats with the heading last, bit j = bev_iou > thresh[0] (nms_mask_kernel of nms.hip).  j > i only.
template <bool CIRCLE>
__global__ __launch_bounds__(64) void nms_batched_mask_kernel(const float *__restrict__ rows, int stride, const int32_t *__restrict__ offsets,
                                                              const int32_t *__restrict__ counts, int max_count, int64_t total,
                                                              const float *__restrict__ thresh_seg, float thresh_all,
                                                              unsigned long long *__restrict__ mask) {
    constexpr int E = CIRCLE ? 2 : 7;
    __shared__ float col[64 * E];
    const Segment s = segment_of(offsets, counts, blockIdx.z, max_count, total, mask);
    const int rb = blockIdx.y, cb = blockIdx.x, t = threadIdx.x;
    if (rb >= s.col_blocks || cb >= s.col_blocks) return;
    if (cb < rb) return;   // strictly lower tiles carry no bits and are never read: the walk of row i starts at word i / 64
    const float thresh = CIRCLE ? thresh_seg[blockIdx.z] : thresh_all;
    auto stage = [&](int row, float *dst) {
        const float *src = rows + (s.off + row) * stride;
        if constexpr (CIRCLE) {
            dst[0] = src[0];
            dst[1] = src[1];
        } else {
            for (int e = 0; e < 6; ++e) dst[e] = src[e];
            dst[6] = src[stride - 1];
        }
    };
    const int cj = cb * 64 + t;
    if (cj < s.n) stage(cj, col + t * E);
    __syncthreads();
    const int ri = rb * 64 + t;
    if (ri >= s.n) return;
    float mine[E];
    stage(ri, mine);
    const int ncol = min(64, s.n - cb * 64);
    unsigned long long bits = 0ull;
    for (int j = (rb == cb ? t + 1 : 0); j < ncol; ++j) {
        bool hit;
        if constexpr (CIRCLE) {
            const float dx = mine[0] - col[j * 2], dy = mine[1] - col[j * 2 + 1];
            hit = dx * dx + dy * dy <= thresh;   // the reference's expression, no FMA contraction
        } else {
            hit = bev_iou(mine, col + j * 7) > thresh;
        }
        if (hit) bits |= 1ull << j;
    }
    s.mask[(int64_t)ri * s.col_blocks + cb] = bits;
}

// the greedy walk of nms_select_kernel (nms.hip), one workgroup per segment; n_keep[seg] is written for every segment
__global__ __launch_bounds__(256) void nms_batched_select_kernel(const int32_t *__restrict__ offsets, const int32_t *__restrict__ counts, int max_count,
                                                                 int64_t total, unsigned long long *__restrict__ mask, int max_keep,
                                                                 int64_t *__restrict__ keep, int32_t *__restrict__ n_keep) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long removed[];   // [ceil(max_count / 64)] bits, then two ints
    const int seg = blockIdx.x;
    if (max_keep <= 0 || max_count <= 0) {
        if (threadIdx.x == 0) n_keep[seg] = 0;
        return;
    }
    const Segment s = segment_of(offsets, counts, seg, max_count, total, mask);
    int *count = (int *)(removed + (max_count + 63) / 64), *alive = count + 1;
    for (int e = threadIdx.x; e < s.col_blocks; e += 256) removed[e] = 0ull;
    if (threadIdx.x == 0) *count = 0;
    __syncthreads();
    keep += (int64_t)seg * max_keep;
    for (int i = 0; i < s.n; ++i) {
        if (threadIdx.x == 0) *alive = !((removed[i >> 6] >> (i & 63)) & 1ull);
        __syncthreads();
        if (*alive) {
            if (threadIdx.x == 0) {
                if (*count < max_keep) keep[*count] = i;
                ++*count;
            }
            for (int e = (i >> 6) + threadIdx.x; e < s.col_blocks; e += 256) removed[e] |= s.mask[(int64_t)i * s.col_blocks + e];
        }
        __syncthreads();
        if (*count >= max_keep) break;   // uniform: count is shared and settled by the barrier
    }
    if (threadIdx.x == 0) n_keep[seg] = *count < max_keep ? *count : max_keep;
}

// ---- fixed-capacity assembly ----------------------------------------------------------------------------------------------------------
// One workgroup per sample: the kept rows of its segments (task * samples + sample) in task order, as predict_on_device's gather lays
// them out, into slots of tasks * max_keep rows; the rows behind the sample's count are written as well (zero boxes and scores, label
// -1), so the outputs are defined everywhere.  A kept index outside the packed list (a wrong device array) gives such a padding row.
__global__ __launch_bounds__(256) void predict_static_gather_kernel(const float *__restrict__ cand_boxes, const float *__restrict__ cand_scores,
                                                                    const int64_t *__restrict__ cand_labels, const int32_t *__restrict__ offsets,
                                                                    const int64_t *__restrict__ keep, const int32_t *__restrict__ n_keep, int tasks,
                                                                    int samples, int max_keep, int box_dim, int64_t total, float *__restrict__ boxes,
                                                                    float *__restrict__ scores, int64_t *__restrict__ labels,
                                                                    int32_t *__restrict__ counts) {
    const int b = blockIdx.x;
    const int64_t cap = (int64_t)tasks * max_keep;
    float *out_boxes = boxes + b * cap * box_dim, *out_scores = scores + b * cap;
    int64_t *out_labels = labels + b * cap;
    int64_t count = 0;
    for (int t = 0; t < tasks; ++t) {
        const int seg = t * samples + b;
        const int n = min(max(n_keep[seg], 0), max_keep);
        const int64_t off = offsets[seg];
        for (int i = threadIdx.x; i < n; i += 256) {
            int64_t row = off + keep[(int64_t)seg * max_keep + i];
            if (row < 0 || row >= total || off < 0) row = -1;
            float *dst = out_boxes + (count + i) * box_dim;
            for (int c = 0; c < box_dim; ++c) dst[c] = row < 0 ? 0.f : cand_boxes[row * box_dim + c];
            out_scores[count + i] = row < 0 ? 0.f : cand_scores[row];
            out_labels[count + i] = row < 0 ? -1 : cand_labels[row];
        }
        count += n;
    }
    for (int64_t i = count + threadIdx.x; i < cap; i += 256) {
        for (int c = 0; c < box_dim; ++c) out_boxes[i * box_dim + c] = 0.f;
        out_scores[i] = 0.f;
        out_labels[i] = -1;
    }
    if (threadIdx.x == 0) counts[b] = (int32_t)count;
}

static int check_tasks(const char *what, const s2d_center_predict_task *tasks, int num_tasks, int samples, int h, int w, PredictTasks &out) {
    S2D_CHECK_ARG(tasks, "%s: null task table", what);
    S2D_CHECK_ARG(num_tasks >= 1 && num_tasks <= CP_MAX_TASKS, "%s: %d tasks (1..%d supported)", what, num_tasks, CP_MAX_TASKS);
    S2D_CHECK_ARG(samples >= 0 && h >= 0 && w >= 0, "%s: negative size (samples %d, h %d, w %d)", what, samples, h, w);
    S2D_CHECK_ARG((int64_t)h * w < (1ll << 31) && (int64_t)num_tasks * samples <= 65535, "%s: map or segment count too large", what);
    for (int i = 0; i < num_tasks; ++i) {
        const s2d_center_predict_task &t = tasks[i];
        S2D_CHECK_ARG(t.classes >= 1, "%s: task %d has %d classes", what, i, t.classes);
        S2D_CHECK_ARG((t.map[M_VEL] != nullptr) == (tasks[0].map[M_VEL] != nullptr), "%s: task %d: vel on some tasks only", what, i);
        for (int m = 0; m < 6; ++m) {
            S2D_CHECK_ARG(t.map[m] || m == M_VEL, "%s: task %d: null map %d", what, i, m);
            S2D_CHECK_ARG(t.channel_stride[m] >= 0 && t.pixel_stride[m] >= 0, "%s: task %d: negative stride of map %d", what, i, m);
        }
        out.t[i] = t;
    }
    for (int i = num_tasks; i < CP_MAX_TASKS; ++i) out.t[i] = tasks[0];
    return S2D_OK;
}

}  // namespace s2d

using namespace s2d;

extern "C" int s2d_center_predict_score(const s2d_center_predict_task *tasks, int num_tasks, int samples, int h, int w, int double_flip,
                                        float score_threshold, const float *range6, float out_size_factor, float voxel_x, float voxel_y, float pc_x,
                                        float pc_y, float *score, int32_t *label, int32_t *count, s2d_stream_t stream) {
    PredictTasks pt;
    const int rc = check_tasks("center_predict_score", tasks, num_tasks, samples, h, w, pt);
    if (rc != S2D_OK) return rc;
    const int64_t segs = (int64_t)num_tasks * samples, hw = (int64_t)h * w;
    if (segs == 0) return S2D_OK;
    S2D_CHECK_ARG(count, "center_predict_score: null count");
    hipStream_t st = (hipStream_t)stream;
    const int zrc = zero_async(count, (size_t)segs * sizeof(int32_t), st);
    if (zrc != S2D_OK) return zrc;
    if (hw == 0) return S2D_OK;
    S2D_CHECK_ARG(score && label, "center_predict_score: null output");
    ScoreArgs a{score_threshold, range6 != nullptr, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    for (int k = 0; k < 3 && range6; ++k) {
        a.lo[k] = range6[k];
        a.hi[k] = range6[3 + k];
    }
    const PredictGeo g{samples, h, w, double_flip != 0, out_size_factor, voxel_x, voxel_y, pc_x, pc_y};
    hipLaunchKernelGGL(center_score_kernel, dim3((unsigned)ceil_div(hw, 256), (unsigned)segs), dim3(256), 0, st, pt, g, a, score, label, count);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_center_predict_boxes(const s2d_center_predict_task *tasks, int num_tasks, int samples, int h, int w, int double_flip,
                                        float out_size_factor, float voxel_x, float voxel_y, float pc_x, float pc_y, const int64_t *order,
                                        const float *score_sorted, const int32_t *label, const int32_t *offsets, const int32_t *counts, int max_count,
                                        int64_t total, float *boxes, float *scores, int64_t *labels, s2d_stream_t stream) {
    PredictTasks pt;
    const int rc = check_tasks("center_predict_boxes", tasks, num_tasks, samples, h, w, pt);
    if (rc != S2D_OK) return rc;
    S2D_CHECK_ARG(max_count >= 0 && total >= 0, "center_predict_boxes: negative size (max_count %d, total %lld)", max_count, (long long)total);
    const int64_t segs = (int64_t)num_tasks * samples;
    if (segs == 0 || max_count == 0 || total == 0) return S2D_OK;
    S2D_CHECK_ARG(order && score_sorted && label && offsets && counts && boxes && scores && labels, "center_predict_boxes: null argument");
    const PredictGeo g{samples, h, w, double_flip != 0, out_size_factor, voxel_x, voxel_y, pc_x, pc_y};
    hipLaunchKernelGGL(center_boxes_kernel, dim3((unsigned)ceil_div(max_count, 256), (unsigned)segs), dim3(256), 0, (hipStream_t)stream, pt, g, order,
                       score_sorted, label, offsets, counts, max_count, total, pt.t[0].map[M_VEL] ? 9 : 7, boxes, scores, labels);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" size_t s2d_nms_batched_workspace_bytes(int64_t total, int max_count) {
    if (total <= 0 || max_count <= 0) return 256;
    return align_up((size_t)total * ((max_count + 63) / 64) * sizeof(unsigned long long), 256);
}

template <bool CIRCLE>
static int nms_batched(const char *what, const float *rows, int stride, const int32_t *offsets, const int32_t *counts, int segments, int max_count,
                       int64_t total, const float *thresh_seg, float thresh_all, int max_keep, int64_t *keep, int32_t *n_keep, void *ws,
                       size_t ws_bytes, s2d_stream_t stream) {
    S2D_CHECK_ARG(segments >= 0 && segments <= 65535, "%s: %d segments (0..65535)", what, segments);
    S2D_CHECK_ARG(max_count >= 0 && max_count <= 65536, "%s: max_count %d (0..65536)", what, max_count);
    S2D_CHECK_ARG(total >= 0 && max_keep >= 0, "%s: negative size (total %lld, max_keep %d)", what, (long long)total, max_keep);
    S2D_CHECK_ARG(stride >= (CIRCLE ? 2 : 7), "%s: row stride %d", what, stride);
    if (segments == 0) return S2D_OK;
    S2D_CHECK_ARG(n_keep && offsets && counts, "%s: null segment arrays or n_keep", what);
    const bool work = total > 0 && max_count > 0 && max_keep > 0;
    if (work) {
        S2D_CHECK_ARG(rows && keep && (!CIRCLE || thresh_seg), "%s: null argument", what);
        if (!ws || ws_bytes < s2d_nms_batched_workspace_bytes(total, max_count)) {
            set_error("%s: workspace too small", what);
            return S2D_ERR_WORKSPACE;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const int cb = (max_count + 63) / 64;
    unsigned long long *mask = (unsigned long long *)ws;
    if (work)
        hipLaunchKernelGGL(nms_batched_mask_kernel<CIRCLE>, dim3(cb, cb, segments), dim3(64), 0, st, rows, stride, offsets, counts, max_count, total,
                           thresh_seg, thresh_all, mask);
    // (without work the select kernel only writes the zero counts: no memset, DESIGN rule 32)
    hipLaunchKernelGGL(nms_batched_select_kernel, dim3(segments), dim3(256), (size_t)cb * sizeof(unsigned long long) + 16, st, offsets, counts,
                       work ? max_count : 0, total, mask, max_keep, keep, n_keep);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_nms_rotated_bev_batched(const float *boxes, int box_stride, const int32_t *offsets, const int32_t *counts, int segments,
                                           int max_count, int64_t total, float iou_threshold, int max_keep, int64_t *keep, int32_t *n_keep, void *ws,
                                           size_t ws_bytes, s2d_stream_t stream) {
    return nms_batched<false>("nms_rotated_bev_batched", boxes, box_stride, offsets, counts, segments, max_count, total, nullptr, iou_threshold,
                              max_keep, keep, n_keep, ws, ws_bytes, stream);
}

extern "C" int s2d_nms_circle_batched(const float *xy, int xy_stride, const int32_t *offsets, const int32_t *counts, int segments, int max_count,
                                      int64_t total, const float *thresh, int max_keep, int64_t *keep, int32_t *n_keep, void *ws, size_t ws_bytes,
                                      s2d_stream_t stream) {
    return nms_batched<true>("nms_circle_batched", xy, xy_stride, offsets, counts, segments, max_count, total, thresh, 0.f, max_keep, keep, n_keep, ws,
                             ws_bytes, stream);
}

extern "C" int s2d_predict_static_gather(const float *cand_boxes, const float *cand_scores, const int64_t *cand_labels, const int32_t *offsets,
                                         const int64_t *keep, const int32_t *n_keep, int tasks, int samples, int max_keep, int box_dim, int64_t total,
                                         float *boxes, float *scores, int64_t *labels, int32_t *counts, s2d_stream_t stream) {
    S2D_CHECK_ARG(tasks >= 1 && tasks <= CP_MAX_TASKS, "predict_static_gather: %d tasks (1..%d supported)", tasks, CP_MAX_TASKS);
    S2D_CHECK_ARG(samples >= 0 && samples <= 65535 && max_keep >= 0 && total >= 0, "predict_static_gather: bad size (samples %d, max_keep %d, total %lld)",
                  samples, max_keep, (long long)total);
    S2D_CHECK_ARG(box_dim == 7 || box_dim == 9, "predict_static_gather: box_dim %d (7 or 9)", box_dim);
    if (samples == 0) return S2D_OK;
    S2D_CHECK_ARG(offsets && n_keep && counts, "predict_static_gather: null segment arrays or counts");
    S2D_CHECK_ARG(max_keep == 0 || (cand_boxes && cand_scores && cand_labels && keep && boxes && scores && labels), "predict_static_gather: null argument");
    hipLaunchKernelGGL(predict_static_gather_kernel, dim3((unsigned)samples), dim3(256), 0, (hipStream_t)stream, cand_boxes, cand_scores, cand_labels,
                       offsets, keep, n_keep, tasks, samples, max_keep, box_dim, total, boxes, scores, labels, counts);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
