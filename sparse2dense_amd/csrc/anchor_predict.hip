// MultiGroupHead.predict on the device (det3d/models/bbox_heads/mg_head.py:697-1086, single-class rotated-NMS branch): every
// (task, sample) pair - a SEGMENT, segment = task * samples + sample - of a head goes through five launches instead of a dense decode of
// all anchors and a torch chain per segment.
//   anchor_score_kernel    all tasks, all samples: sigmoid class maximum + class, `score >= threshold` -> score map (-1 = dropped or
//                          padding: a sigmoid is never negative), label map, pass count per segment.  The dense [B, A, 7] box tensor of
//                          the chain is never formed.
//   (torch.sort of the score maps, one host read of the counts)
//   anchor_boxes_kernel    decodes the n_s best anchors of every segment into one packed list in the NMS form (heading negated:
//                          (dx, dy, heading) = (w, l, -r)), with the direction label and the centre-range flag of every row
//   (s2d_nms_rotated_bev_batched of center_predict.hip, n_keep stays on the device)
//   anchor_finish_kernel   one workgroup per segment walks its keep list: drops the rows outside post_center_limit_range (AFTER the NMS, as
//                          the reference does: a box outside the range still suppresses), restores the heading sign, applies the direction
//                          flip, adds the task's label base and writes the padded per-segment outputs and their count
//   anchor_finish_static_kernel  (the static path, anchor_predict.StaticAnchorPlan: s2d_segment_topk of segment_topk.hip in place of
//                          the sort, no host read) the same finish with one workgroup per SAMPLE: its tasks in task order, compacted
//                          into [samples][tasks * max_keep] outputs whose padding rows are written too
// The per-task pointers travel by value in the kernel arguments (s2d_anchor_predict_task[8]).  The decode expressions are the ones of
// anchor_decode_kernel (anchor_decode.h); the library is built with -ffp-contract=off, so both paths give the same bits.
// Built without the SLP vectoriser (DESIGN rule 36), as center_predict.hip is: predict may run beside a side stream's MFMA kernels.
#include "anchor_decode.h"

namespace s2d {

constexpr int AP_MAX_TASKS = S2D_ANCHOR_PREDICT_MAX_TASKS;

struct AnchorTasks {
    s2d_anchor_predict_task t[AP_MAX_TASKS];
};

struct AnchorRange {
    int on;
    float lo[3], hi[3];
};

__global__ __launch_bounds__(256) void anchor_score_kernel(AnchorTasks tasks, int samples, int64_t max_anchors, float threshold,
                                                           float *__restrict__ score, int32_t *__restrict__ label, int32_t *__restrict__ count) {
    const int seg = blockIdx.y, task = seg / samples, b = seg % samples;
    const s2d_anchor_predict_task &t = tasks.t[task];
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool pass = false;
    if (a < max_anchors) {
        float s = -1.f;
        int cls = 0;
        if (a < t.num_anchors) {
            const float best = anchor_class_max(t.cls_preds + ((int64_t)b * t.num_anchors + a) * t.classes, t.classes, cls);
            pass = best >= threshold;   // false for a NaN maximum, as in anchor_decode_kernel
            if (pass) s = best;
        }
        score[(int64_t)seg * max_anchors + a] = s;
        label[(int64_t)seg * max_anchors + a] = cls;
    }
    // one atomic per wave: the lanes that pass are counted by a ballot
    const unsigned long long votes = __ballot(pass);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(&count[seg], (int32_t)__popcll(votes));
}

__global__ __launch_bounds__(256) void anchor_boxes_kernel(AnchorTasks tasks, int samples, int64_t max_anchors, AnchorRange rng,
                                                           const int64_t *__restrict__ order, const float *__restrict__ score_sorted,
                                                           const int32_t *__restrict__ label, const int32_t *__restrict__ offsets,
                                                           const int32_t *__restrict__ counts, int max_count, int64_t total,
                                                           float *__restrict__ boxes, float *__restrict__ scores, int32_t *__restrict__ labels,
                                                           int32_t *__restrict__ dirs, uint8_t *__restrict__ in_range) {
    const int seg = blockIdx.y, task = seg / samples, b = seg % samples;
    const s2d_anchor_predict_task &t = tasks.t[task];
    const int64_t rank = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = min((int64_t)min(counts[seg], max_count), t.num_anchors), off = offsets[seg];
    if (rank >= n || off < 0 || off + n > total) return;
    const int64_t a = order[(int64_t)seg * max_anchors + rank];
    if (a < 0 || a >= t.num_anchors) return;
    const int64_t at = (int64_t)b * t.num_anchors + a, row = off + rank;
    float o[7];
    anchor_box_decode(t.box_preds + at * 7, t.anchors + a * 7, o);
    float *bx = boxes + row * 7;
#pragma unroll
    for (int e = 0; e < 6; ++e) bx[e] = o[e];
    bx[6] = -o[6];   // the NMS form; anchor_finish_kernel negates it back (exact)
    scores[row] = score_sorted[(int64_t)seg * max_anchors + rank];
    labels[row] = label[(int64_t)seg * max_anchors + a];
    dirs[row] = t.dir_cls_preds ? (t.dir_cls_preds[at * 2 + 1] > t.dir_cls_preds[at * 2] ? 1 : 0) : 0;
    bool in = true;
    if (rng.on) in = o[0] >= rng.lo[0] && o[1] >= rng.lo[1] && o[2] >= rng.lo[2] && o[0] <= rng.hi[0] && o[1] <= rng.hi[1] && o[2] <= rng.hi[2];
    in_range[row] = in ? 1 : 0;
}

struct AnchorFinish {
    int samples, max_keep, use_dir;
    float dir_offset;
    int label_base[AP_MAX_TASKS];
};

// One kept row of the packed lists -> row `out` of the outputs: the heading sign restored, the direction flip, the task's label base.
// anchor_finish_kernel and anchor_finish_static_kernel both call it, so the two give the same bits.
__device__ __forceinline__ void anchor_finish_row(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                  const int32_t *__restrict__ labels, const int32_t *__restrict__ dirs, int64_t row,
                                                  const AnchorFinish &g, int base_label, int64_t out, float *__restrict__ out_boxes,
                                                  float *__restrict__ out_scores, int64_t *__restrict__ out_labels) {
    const float *bx = boxes + row * 7;
    float *o = out_boxes + out * 7;
#pragma unroll
    for (int e = 0; e < 6; ++e) o[e] = bx[e];
    float r = -bx[6];
    if (g.use_dir) {   // mg_head.py:1057-1066: the heading and the direction classifier disagree -> the opposite heading
        const bool opposite = ((r - g.dir_offset) > 0.f) != (dirs[row] != 0);
        r = r + (opposite ? (float)3.141592653589793 : 0.f);
    }
    o[6] = r;
    out_scores[out] = scores[row];
    out_labels[out] = (int64_t)labels[row] + base_label;
}

__global__ __launch_bounds__(256) void anchor_finish_kernel(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                            const int32_t *__restrict__ labels, const int32_t *__restrict__ dirs,
                                                            const uint8_t *__restrict__ in_range, const int32_t *__restrict__ offsets,
                                                            const int32_t *__restrict__ counts, int64_t total, const int64_t *__restrict__ keep,
                                                            const int32_t *__restrict__ n_keep, AnchorFinish g, float *__restrict__ out_boxes,
                                                            float *__restrict__ out_scores, int64_t *__restrict__ out_labels,
                                                            int32_t *__restrict__ out_count) {
    __shared__ int wave_total[4];
    const int seg = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t off = offsets[seg];
    int rows = counts[seg], n = min(n_keep[seg], g.max_keep);
    if (rows < 0 || off < 0 || off + rows > total) rows = 0;   // a segment outside the packed lists counts as empty
    if (rows == 0 || n < 0) n = 0;
    const int base_label = g.label_base[seg / g.samples];
    int written = 0;   // uniform over the block
    for (int start = 0; start < n; start += 256) {
        const int i = start + threadIdx.x;
        int64_t row = -1;
        if (i < n) {
            const int64_t k = keep[(int64_t)seg * g.max_keep + i];
            if (k >= 0 && k < rows) row = off + k;
        }
        const bool stay = row >= 0 && in_range[row] != 0;
        // order-preserving compaction of the chunk: lanes below me in my wave, plus the waves below mine
        const unsigned long long votes = __ballot(stay);
        const int before = (int)__popcll(votes & ((1ull << lane) - 1ull));
        __syncthreads();   // (the previous chunk's reads of wave_total are done)
        if (lane == 0) wave_total[wave] = (int)__popcll(votes);
        __syncthreads();
        int pos = written + before;
        for (int w = 0; w < wave; ++w) pos += wave_total[w];
        if (stay)
            anchor_finish_row(boxes, scores, labels, dirs, row, g, base_label, (int64_t)seg * g.max_keep + pos, out_boxes, out_scores, out_labels);
        written += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    }
    if (threadIdx.x == 0) out_count[seg] = written;
}

// The finish of the static path (anchor_predict.StaticAnchorPlan): one workgroup per SAMPLE walks its tasks in task order, every segment
// as anchor_finish_kernel walks it, and compacts the surviving rows from row 0 of the sample's cap = tasks * max_keep output rows - the
// write position is carried on across the tasks.  The rows behind the sample's count are written as well (zero boxes and scores, label
// -1), so the outputs are a function of the inputs alone.  No atomics, no communication between workgroups.
__global__ __launch_bounds__(256) void anchor_finish_static_kernel(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                                   const int32_t *__restrict__ labels, const int32_t *__restrict__ dirs,
                                                                   const uint8_t *__restrict__ in_range, const int32_t *__restrict__ offsets,
                                                                   const int32_t *__restrict__ counts, int64_t total,
                                                                   const int64_t *__restrict__ keep, const int32_t *__restrict__ n_keep,
                                                                   AnchorFinish g, int num_tasks, float *__restrict__ out_boxes,
                                                                   float *__restrict__ out_scores, int64_t *__restrict__ out_labels,
                                                                   int32_t *__restrict__ out_counts) {
    __shared__ int wave_total[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cap = (int64_t)num_tasks * g.max_keep, first = b * cap;
    int written = 0;   // uniform over the block; at most cap: every segment adds at most max_keep
    for (int task = 0; task < num_tasks; ++task) {
        const int seg = task * g.samples + b;
        const int64_t off = offsets[seg];
        int rows = counts[seg], n = min(n_keep[seg], g.max_keep);
        if (rows < 0 || off < 0 || off + rows > total) rows = 0;   // a segment outside the packed lists counts as empty
        if (rows == 0 || n < 0) n = 0;
        const int base_label = g.label_base[task];
        for (int start = 0; start < n; start += 256) {
            const int i = start + threadIdx.x;
            int64_t row = -1;
            if (i < n) {
                const int64_t k = keep[(int64_t)seg * g.max_keep + i];
                if (k >= 0 && k < rows) row = off + k;
            }
            const bool stay = row >= 0 && in_range[row] != 0;
            const unsigned long long votes = __ballot(stay);
            const int before = (int)__popcll(votes & ((1ull << lane) - 1ull));
            __syncthreads();   // (the previous chunk's reads of wave_total are done)
            if (lane == 0) wave_total[wave] = (int)__popcll(votes);
            __syncthreads();
            int pos = written + before;
            for (int w = 0; w < wave; ++w) pos += wave_total[w];
            if (stay) anchor_finish_row(boxes, scores, labels, dirs, row, g, base_label, first + pos, out_boxes, out_scores, out_labels);
            written += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        }
    }
    for (int64_t i = written + threadIdx.x; i < cap; i += 256) {
        float *o = out_boxes + (first + i) * 7;
#pragma unroll
        for (int e = 0; e < 7; ++e) o[e] = 0.f;
        out_scores[first + i] = 0.f;
        out_labels[first + i] = -1;
    }
    if (threadIdx.x == 0) out_counts[b] = written;
}

static int check_anchor_tasks(const char *what, const s2d_anchor_predict_task *tasks, int num_tasks, int samples, int64_t max_anchors,
                              AnchorTasks &out) {
    S2D_CHECK_ARG(tasks, "%s: null task table", what);
    S2D_CHECK_ARG(num_tasks >= 1 && num_tasks <= AP_MAX_TASKS, "%s: %d tasks (1..%d supported)", what, num_tasks, AP_MAX_TASKS);
    S2D_CHECK_ARG(samples >= 0 && max_anchors >= 0, "%s: negative size (samples %d, max_anchors %lld)", what, samples, (long long)max_anchors);
    S2D_CHECK_ARG(max_anchors < (1ll << 31) && (int64_t)num_tasks * samples <= 65535, "%s: anchor or segment count too large", what);
    for (int i = 0; i < num_tasks; ++i) {
        const s2d_anchor_predict_task &t = tasks[i];
        S2D_CHECK_ARG(t.classes >= 1, "%s: task %d has %d classes", what, i, t.classes);
        S2D_CHECK_ARG(t.num_anchors >= 0 && t.num_anchors <= max_anchors, "%s: task %d has %lld anchors (max_anchors %lld)", what, i,
                      (long long)t.num_anchors, (long long)max_anchors);
        S2D_CHECK_ARG(t.num_anchors == 0 || samples == 0 || (t.box_preds && t.cls_preds && t.anchors), "%s: task %d: null input", what, i);
        out.t[i] = t;
    }
    for (int i = num_tasks; i < AP_MAX_TASKS; ++i) out.t[i] = tasks[0];
    return S2D_OK;
}

}  // namespace s2d

using namespace s2d;

extern "C" int s2d_anchor_predict_score(const s2d_anchor_predict_task *tasks, int num_tasks, int samples, int64_t max_anchors,
                                        float score_threshold, float *score, int32_t *label, int32_t *count, s2d_stream_t stream) {
    AnchorTasks at;
    const int rc = check_anchor_tasks("anchor_predict_score", tasks, num_tasks, samples, max_anchors, at);
    if (rc != S2D_OK) return rc;
    const int64_t segs = (int64_t)num_tasks * samples;
    if (segs == 0) return S2D_OK;
    S2D_CHECK_ARG(count, "anchor_predict_score: null count");
    S2D_CHECK_ARG(max_anchors == 0 || (score && label), "anchor_predict_score: null output");
    hipStream_t st = (hipStream_t)stream;
    if (int zrc = zero_async(count, (size_t)segs * sizeof(int32_t), st)) return zrc;   // (a kernel, not a memset node: DESIGN rule 32)
    if (max_anchors > 0)
        hipLaunchKernelGGL(anchor_score_kernel, dim3((unsigned)ceil_div(max_anchors, 256), (unsigned)segs), dim3(256), 0, st, at, samples,
                           max_anchors, score_threshold, score, label, count);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_anchor_predict_boxes(const s2d_anchor_predict_task *tasks, int num_tasks, int samples, int64_t max_anchors,
                                        const float *range6, const int64_t *order, const float *score_sorted, const int32_t *label,
                                        const int32_t *offsets, const int32_t *counts, int max_count, int64_t total, float *boxes, float *scores,
                                        int32_t *labels, int32_t *dir_labels, uint8_t *in_range, s2d_stream_t stream) {
    AnchorTasks at;
    const int rc = check_anchor_tasks("anchor_predict_boxes", tasks, num_tasks, samples, max_anchors, at);
    if (rc != S2D_OK) return rc;
    S2D_CHECK_ARG(max_count >= 0 && total >= 0, "anchor_predict_boxes: negative size (max_count %d, total %lld)", max_count, (long long)total);
    const int64_t segs = (int64_t)num_tasks * samples;
    if (segs == 0 || max_count == 0 || total == 0 || max_anchors == 0) return S2D_OK;
    S2D_CHECK_ARG(order && score_sorted && label && offsets && counts, "anchor_predict_boxes: null input");
    S2D_CHECK_ARG(boxes && scores && labels && dir_labels && in_range, "anchor_predict_boxes: null output");
    AnchorRange rng{range6 != nullptr, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    for (int k = 0; k < 3 && range6; ++k) {
        rng.lo[k] = range6[k];
        rng.hi[k] = range6[3 + k];
    }
    hipLaunchKernelGGL(anchor_boxes_kernel, dim3((unsigned)ceil_div(max_count, 256), (unsigned)segs), dim3(256), 0, (hipStream_t)stream, at, samples,
                       max_anchors, rng, order, score_sorted, label, offsets, counts, max_count, total, boxes, scores, labels, dir_labels, in_range);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_anchor_predict_finish(const s2d_anchor_predict_task *tasks, int num_tasks, int samples, const float *boxes,
                                         const float *scores, const int32_t *labels, const int32_t *dir_labels, const uint8_t *in_range,
                                         const int32_t *offsets, const int32_t *counts, int64_t total, const int64_t *keep,
                                         const int32_t *n_keep, int max_keep, int use_direction, float direction_offset, float *out_boxes, float *out_scores,
                                         int64_t *out_labels, int32_t *out_count, s2d_stream_t stream) {
    S2D_CHECK_ARG(tasks, "anchor_predict_finish: null task table");
    S2D_CHECK_ARG(num_tasks >= 1 && num_tasks <= AP_MAX_TASKS, "anchor_predict_finish: %d tasks (1..%d supported)", num_tasks, AP_MAX_TASKS);
    S2D_CHECK_ARG(samples >= 0 && (int64_t)num_tasks * samples <= 65535, "anchor_predict_finish: bad samples %d", samples);
    S2D_CHECK_ARG(total >= 0 && max_keep >= 0, "anchor_predict_finish: negative size (total %lld, max_keep %d)", (long long)total, max_keep);
    const int segs = num_tasks * samples;
    if (segs == 0) return S2D_OK;
    S2D_CHECK_ARG(offsets && counts && n_keep && out_count, "anchor_predict_finish: null segment arrays or out_count");
    S2D_CHECK_ARG(max_keep == 0 || total == 0 || (boxes && scores && labels && dir_labels && in_range && keep),
                  "anchor_predict_finish: null input");
    S2D_CHECK_ARG(max_keep == 0 || total == 0 || (out_boxes && out_scores && out_labels), "anchor_predict_finish: null output");
    AnchorFinish g{samples, total == 0 ? 0 : max_keep, use_direction != 0, direction_offset, {0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; i < num_tasks; ++i) g.label_base[i] = tasks[i].label_base;
    hipLaunchKernelGGL(anchor_finish_kernel, dim3((unsigned)segs), dim3(256), 0, (hipStream_t)stream, boxes, scores, labels, dir_labels, in_range,
                       offsets, counts, total, keep, n_keep, g, out_boxes, out_scores, out_labels, out_count);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_anchor_predict_finish_static(const s2d_anchor_predict_task *tasks, int num_tasks, int samples, const float *boxes,
                                                const float *scores, const int32_t *labels, const int32_t *dir_labels, const uint8_t *in_range,
                                                const int32_t *offsets, const int32_t *counts, int64_t total, const int64_t *keep,
                                                const int32_t *n_keep, int max_keep, int use_direction, float direction_offset, float *out_boxes,
                                                float *out_scores, int64_t *out_labels, int32_t *out_counts, s2d_stream_t stream) {
    S2D_CHECK_ARG(tasks, "anchor_predict_finish_static: null task table");
    S2D_CHECK_ARG(num_tasks >= 1 && num_tasks <= AP_MAX_TASKS, "anchor_predict_finish_static: %d tasks (1..%d supported)", num_tasks, AP_MAX_TASKS);
    S2D_CHECK_ARG(samples >= 0 && (int64_t)num_tasks * samples <= 65535, "anchor_predict_finish_static: bad samples %d", samples);
    S2D_CHECK_ARG(total >= 0 && max_keep >= 0, "anchor_predict_finish_static: negative size (total %lld, max_keep %d)", (long long)total, max_keep);
    if (samples == 0) return S2D_OK;
    S2D_CHECK_ARG(offsets && counts && n_keep && out_counts, "anchor_predict_finish_static: null segment arrays or out_counts");
    S2D_CHECK_ARG(boxes && scores && labels && dir_labels && in_range && keep, "anchor_predict_finish_static: null input");
    S2D_CHECK_ARG(out_boxes && out_scores && out_labels, "anchor_predict_finish_static: null output");
    AnchorFinish g{samples, max_keep, use_direction != 0, direction_offset, {0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; i < num_tasks; ++i) g.label_base[i] = tasks[i].label_base;
    hipLaunchKernelGGL(anchor_finish_static_kernel, dim3((unsigned)samples), dim3(256), 0, (hipStream_t)stream, boxes, scores, labels, dir_labels,
                       in_range, offsets, counts, total, keep, n_keep, g, num_tasks, out_boxes, out_scores, out_labels, out_counts);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
