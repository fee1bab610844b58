// Detection AP evaluation (the reference's KITTI-protocol evaluator: det3d/datasets/kitti/eval.py, det3d/datasets/utils/eval.py over
// rotate_iou_gpu_eval of det3d/ops/nms/nms_gpu.py:580-672).  Three entries, each ONE launch for every frame of the split:
//
//   s2d_eval_overlaps   one thread per (ground truth, detection) pair of a frame, frames found by a binary search in the pair offsets.
//                       metric 0: image boxes in double; metric 1: BEV IoU in fp32 as devRotateIoUEval; metric 2: the fp32 BEV
//                       intersection area, then the reference's height term in double (box3d_overlap_kernel), stored to fp32 as the
//                       reference stores it into `rinc`.
//   s2d_eval_match      compute_statistics_jit with compute_fp=False: one wave per (frame, class, difficulty, overlap index).
//   s2d_eval_pr         compute_statistics_jit with compute_fp=True: one wave per (frame, class, difficulty, overlap index, threshold).
//
// Both matching kernels walk the ground truths of their frame in order - a taken detection is gone for the later ones, so the walk is
// sequential - and the 64 lanes scan the detections (lane l holds detections l, l + 64, ...: at most 16, their flags in three 16-bit
// register masks).  The reference's scan over the detections is one reduction (with min_overlap >= 0, which the host checks):
//   compute_fp=False   the highest score among the candidates with overlap > min_overlap, the lowest index on equal scores (its `>`);
//   compute_fp=True    its three branches take the first non-ignored candidate whether or not an ignored one was taken before (overlap >
//                      max_overlap = 0, or assigned_ignored_det), later non-ignored ones only with a strictly larger overlap, and an ignored
//                      one only while nothing is chosen: the largest overlap among the non-ignored candidates, the lowest index on equal
//                      overlaps, else the first ignored candidate.
// The ignore flags of clean_data are recomputed here from every row's name code, image-box height, occlusion and truncation; they are
// never stored per (class, difficulty).  Scores, thresholds and min_overlap are compared in double, overlaps are fp32 values widened, as
// in the reference.  tp / fp / fn are integers (64-bit integer atomics over the frames): two calls give the same bits.
//
// The rectangle corners are nms_geom.h's (rect_corners) with the rotation negated, which maps the reference's rbbox_to_corners (a corner
// (cx, cy) goes to (cos r cx + sin r cy + x, -sin r cx + cos r cy + y)) onto it.  The intersection is NOT nms_geom.h's bev_overlap: that
// one is pinned to the reference's CPU IoU for NMS, whose inside test accepts corners up to 1e-2 outside the other rectangle, and on the
// evaluator's pairs it is off by up to 1.7e-2 m^2 where the evaluator's own fp32 triangle fan is within 4e-5 of the exact overlap.  Here
// one rectangle is clipped against the four edges of the other (Sutherland-Hodgman on rect_corners / cross2, fp32, at most 8 vertices)
// and the area is the shoelace sum: within 1.2e-5 m^2 on the same pairs.
#include <limits.h>

#include "nms_geom.h"

namespace s2d {
namespace {

constexpr int EV_ROWS = S2D_EVAL_MAX_ROWS;
constexpr int EV_SLOTS = EV_ROWS / 64;
constexpr int EV_PTS = S2D_EVAL_SAMPLE_PTS;
constexpr double EV_NO_DETECTION = -10000000.0;
constexpr int EV_VAN = 11, EV_SITTING = 12, EV_DONTCARE = 256;   // row name codes beyond the class table (evaluation.name_codes)
static_assert(EV_SLOTS <= 32, "a lane's detections are bits of one 32-bit mask");

struct EvRows {
    const float *ov;          // ragged: frame f at ov_off[f], [ng][nd]
    const double *det_img;    // [rows][4]
    const double *det_score;  // [rows]
    const int32_t *det_name;
    const double *gt_img;     // [rows][4]
    const double *gt_occ;     // [rows][2] = occluded, truncated
    const int32_t *gt_name;
    const int32_t *det_off, *gt_off;   // [frames + 1]
    const int64_t *ov_off;             // [frames + 1]
};

struct EvTable {
    int classes[S2D_EVAL_MAX_CLASSES];
    int diffs[3];
    int num_classes, num_diffs, num_ov;
    const double *min_ov;   // [num_classes][num_ov]
};

struct EvFrame {
    int nd, ng, stride, d0, g0;
    const float *ov;
};

__device__ __forceinline__ EvFrame ev_frame(const EvRows &r, int f) {
    EvFrame fr;
    fr.d0 = r.det_off[f];
    fr.g0 = r.gt_off[f];
    fr.stride = r.det_off[f + 1] - fr.d0;
    const int ng = r.gt_off[f + 1] - fr.g0;
    fr.nd = fr.stride < 0 ? 0 : fr.stride > EV_ROWS ? EV_ROWS : fr.stride;   // (the host sends frames above the limit to its own route)
    fr.ng = ng < 0 ? 0 : ng > EV_ROWS ? EV_ROWS : ng;
    fr.ov = r.ov + r.ov_off[f];
    return fr;
}

__device__ __forceinline__ double ev_min_height(int diff) { return diff == 0 ? 40.0 : 25.0; }

// clean_data's flag of ground-truth row g for class cls at difficulty diff: 0 counted, 1 ignored, -1 another class
__device__ __forceinline__ int ev_gt_ignored(const EvRows &r, int g, int cls, int diff) {
    const int code = r.gt_name[g] & 255;
    const int valid = code == cls ? 1 : ((cls == 1 && code == EV_SITTING) || (cls == 0 && code == EV_VAN)) ? 0 : -1;
    const double height = r.gt_img[(size_t)g * 4 + 3] - r.gt_img[(size_t)g * 4 + 1];
    const double max_trunc = diff == 0 ? 0.15 : diff == 1 ? 0.3 : 0.5;
    const bool ignore = r.gt_occ[(size_t)g * 2] > (double)diff || r.gt_occ[(size_t)g * 2 + 1] > max_trunc || height <= ev_min_height(diff);
    if (valid == 1 && !ignore) return 0;
    if (valid == 0 || (ignore && valid == 1)) return 1;
    return -1;
}

// One frame's walk for one (class, difficulty, min_overlap[, threshold]).  FP = compute_fp.  Every lane of the wave runs this with the
// same arguments; tp, fp, fn and nvalid come back wave-uniform.
template <bool FP>
__device__ __forceinline__ void ev_walk(const EvRows &r, const EvFrame &fr, int cls, int diff, double min_ov, double thresh, int metric,
                                        double *tp_out, int &tp, int &fp, int &fn, int &nvalid) {
    const int lane = threadIdx.x & 63;
    const double min_h = ev_min_height(diff);
    unsigned alive = 0, ign1 = 0, assigned = 0;   // bit t: detection t * 64 + lane
#pragma unroll
    for (int t = 0; t < EV_SLOTS; ++t) {
        const int j = t * 64 + lane;
        if (j >= fr.nd) continue;
        const double *b = r.det_img + (size_t)(fr.d0 + j) * 4;
        const int flag = fabs(b[3] - b[1]) < min_h ? 1 : ((r.det_name[fr.d0 + j] & 255) == cls ? 0 : -1);
        const bool below = FP && r.det_score[fr.d0 + j] < thresh;   // ignored_threshold
        if (flag != -1 && !below) alive |= 1u << t;
        if (flag == 1) ign1 |= 1u << t;
    }
    tp = fp = fn = nvalid = 0;
    for (int i = 0; i < fr.ng; ++i) {
        const int ig = ev_gt_ignored(r, fr.g0 + i, cls, diff);
        if (ig == 0) ++nvalid;
        if (ig == -1) continue;
        const float *row = fr.ov + (size_t)i * fr.stride;
        const unsigned open = alive & ~assigned;
        double key = FP ? -1.0 : EV_NO_DETECTION;   // FP: the overlap of the chosen non-ignored candidate; else the chosen score
        int idx = INT_MAX, first_ignored = INT_MAX;
#pragma unroll
        for (int t = 0; t < EV_SLOTS; ++t) {
            if (!((open >> t) & 1u)) continue;
            const int j = t * 64 + lane;
            const double o = (double)row[j];
            if (!(o > min_ov)) continue;
            if (!FP) {
                const double s = r.det_score[fr.d0 + j];
                if (s > key) { key = s; idx = j; }
            } else if ((ign1 >> t) & 1u) {
                if (j < first_ignored) first_ignored = j;
            } else if (o > key) {
                key = o;
                idx = j;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double ok = __shfl_xor(key, d, 64);
            const int oi = __shfl_xor(idx, d, 64);
            if (ok > key || (ok == key && oi < idx)) { key = ok; idx = oi; }
            if (FP) {
                const int of = __shfl_xor(first_ignored, d, 64);
                first_ignored = of < first_ignored ? of : first_ignored;
            }
        }
        if (FP && idx == INT_MAX) idx = first_ignored;
        if (idx == INT_MAX) {   // NO_DETECTION
            if (ig == 0) ++fn;
            continue;
        }
        const bool det_ignored = ((__shfl(ign1, idx & 63, 64) >> (idx >> 6)) & 1u) != 0;
        if (!(ig == 1 || det_ignored)) {   // only a true positive adds a threshold
            if (!FP && lane == 0) tp_out[tp] = r.det_score[fr.d0 + idx];
            ++tp;
        }
        if (lane == (idx & 63)) assigned |= 1u << (idx >> 6);
    }
    if (FP) {
        const unsigned rest = alive & ~assigned & ~ign1;
        int n = __popc(rest);
        if (metric == 0) {   // detections inside a DontCare region (image_box_overlap with criterion 0: over the detection's area) are no fp
            for (int t = 0; t < EV_SLOTS; ++t) {
                if (!((rest >> t) & 1u)) continue;
                const double *b = r.det_img + (size_t)(fr.d0 + t * 64 + lane) * 4;
                bool stuff = false;
                for (int i = 0; i < fr.ng && !stuff; ++i) {
                    if (!(r.gt_name[fr.g0 + i] & EV_DONTCARE)) continue;
                    const double *q = r.gt_img + (size_t)(fr.g0 + i) * 4;
                    const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
                    if (!(iw > 0)) continue;
                    const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
                    if (!(ih > 0)) continue;
                    stuff = iw * ih / ((b[2] - b[0]) * (b[3] - b[1])) > min_ov;
                }
                n -= stuff ? 1 : 0;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
        fp = n;
    }
}

__device__ __forceinline__ void ev_combo(const EvTable &tb, int c, int &cls, int &diff, double &min_ov) {
    const int k = c % tb.num_ov, l = (c / tb.num_ov) % tb.num_diffs, m = c / (tb.num_ov * tb.num_diffs);
    cls = tb.classes[m];
    diff = tb.diffs[l];
    min_ov = tb.min_ov[m * tb.num_ov + k];
}

__global__ __launch_bounds__(64) void eval_match_kernel(EvRows r, EvTable tb, int64_t total_gt, double *__restrict__ tp_scores,
                                                        int32_t *__restrict__ counts, int64_t *__restrict__ pr, int pr_len) {
    const int f = blockIdx.x, c = blockIdx.y, combos = gridDim.y, lane = threadIdx.x;
    // the sweep accumulates into pr: cleared here, one launch earlier on the same stream
    for (int64_t i = ((int64_t)f * combos + c) * 64 + lane; i < pr_len; i += (int64_t)gridDim.x * combos * 64) pr[i] = 0;
    int cls, diff;
    double min_ov;
    ev_combo(tb, c, cls, diff, min_ov);
    const EvFrame fr = ev_frame(r, f);
    int tp, fp, fn, nvalid;
    ev_walk<false>(r, fr, cls, diff, min_ov, 0.0, 0, tp_scores + (size_t)c * total_gt + fr.g0, tp, fp, fn, nvalid);
    if (lane == 0) {
        counts[((size_t)f * combos + c) * 2 + 0] = tp;
        counts[((size_t)f * combos + c) * 2 + 1] = nvalid;
    }
}

__global__ __launch_bounds__(64) void eval_pr_kernel(EvRows r, EvTable tb, int metric, const double *__restrict__ thresholds,
                                                     const int32_t *__restrict__ num_thresholds, int64_t *__restrict__ pr) {
    const int f = blockIdx.x, c = blockIdx.y, t = blockIdx.z;
    if (t >= num_thresholds[c]) return;
    int cls, diff;
    double min_ov;
    ev_combo(tb, c, cls, diff, min_ov);
    const EvFrame fr = ev_frame(r, f);
    int tp, fp, fn, nvalid;
    ev_walk<true>(r, fr, cls, diff, min_ov, thresholds[c * EV_PTS + t], metric, nullptr, tp, fp, fn, nvalid);
    if (threadIdx.x == 0) {
        unsigned long long *out = reinterpret_cast<unsigned long long *>(pr) + ((size_t)c * EV_PTS + t) * 3;
        if (tp) atomicAdd(out + 0, (unsigned long long)(long long)tp);
        if (fp) atomicAdd(out + 1, (unsigned long long)(long long)fp);   // (fp can be negative only if a caller hands in inconsistent rows)
        if (fn) atomicAdd(out + 2, (unsigned long long)(long long)fn);
    }
}

// area of the intersection of rectangle a with rectangle b (rows as nms_geom.h reads them)
__device__ __forceinline__ float ev_clip_area(const float *a, const float *b) {
    P2 ca[5], cb[5];
    rect_corners(a, ca);
    rect_corners(b, cb);
    P2 poly[8], next[8];
    int n = 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) poly[k] = ca[k];
    const P2 ctr{b[0], b[1]};
    for (int e = 0; e < 4; ++e) {
        const float sgn = cross2(cb[e + 1], ctr, cb[e]) >= 0 ? 1.f : -1.f;   // the side of the edge b lies on (negative sizes flip the corners)
        int m = 0;
        for (int k = 0; k < n; ++k) {
            const P2 cur = poly[k], nx = poly[k + 1 < n ? k + 1 : 0];
            const float dc = sgn * cross2(cb[e + 1], cur, cb[e]), dn = sgn * cross2(cb[e + 1], nx, cb[e]);
            if (dc >= 0 && m < 8) next[m++] = cur;
            if ((dc >= 0) != (dn >= 0) && m < 8) {   // (a convex polygon gains at most one vertex per edge: 8 is never exceeded in exact arithmetic)
                const float t = dc / (dc - dn);
                next[m++] = P2{cur.x + (nx.x - cur.x) * t, cur.y + (nx.y - cur.y) * t};
            }
        }
        n = m;
        for (int k = 0; k < n; ++k) poly[k] = next[k];
    }
    float area = 0.f;
    for (int k = 1; k + 1 < n; ++k)
        area += (poly[k].x - poly[0].x) * (poly[k + 1].y - poly[0].y) - (poly[k].y - poly[0].y) * (poly[k + 1].x - poly[0].x);
    return fabsf(area) / 2.0f;
}

// the rows of one rectangle as nms_geom.h reads them (x, y, -, dx, dy, -, angle) from a reference row (x, y, dx, dy, r)
__device__ __forceinline__ void ev_bev_row(const double *box, int a0, int a1, float (&out)[7]) {
    out[0] = (float)box[a0];
    out[1] = (float)box[a1];
    out[2] = 0.f;
    out[3] = (float)box[3 + a0];
    out[4] = (float)box[3 + a1];
    out[5] = 0.f;
    out[6] = -(float)box[6];
}

__global__ __launch_bounds__(256) void eval_overlaps_kernel(int metric, const double *__restrict__ det_box, const double *__restrict__ det_img,
                                                            const double *__restrict__ gt_box, const double *__restrict__ gt_img,
                                                            const int32_t *__restrict__ det_off, const int32_t *__restrict__ gt_off,
                                                            const int64_t *__restrict__ ov_off, int frames, int64_t pairs, int z_axis,
                                                            double z_center, float *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    int lo = 0, hi = frames;   // the last frame whose pairs start at or before p (frames without pairs share their start with the next)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ov_off[mid] <= p) lo = mid; else hi = mid;
    }
    const int nd = det_off[lo + 1] - det_off[lo], ng = gt_off[lo + 1] - gt_off[lo];
    const int64_t local = p - ov_off[lo];
    if (nd <= 0 || local < 0 || local >= (int64_t)nd * ng) return;
    const int i = (int)(local / nd), j = (int)(local % nd);
    const size_t g = (size_t)gt_off[lo] + i, d = (size_t)det_off[lo] + j;
    if (metric == 0) {   // image_box_overlap(detections, ground truths), criterion -1
        const double *b = det_img + d * 4, *q = gt_img + g * 4;
        double v = 0.0;
        const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
        if (iw > 0) {
            const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
            if (ih > 0) v = iw * ih / ((b[2] - b[0]) * (b[3] - b[1]) + (q[2] - q[0]) * (q[3] - q[1]) - iw * ih);
        }
        out[p] = (float)v;
        return;
    }
    const int a0 = z_axis == 0 ? 1 : 0, a1 = z_axis == 2 ? 1 : 2;
    const double *bd = det_box + d * 7, *bg = gt_box + g * 7;
    float rd[7], rg[7];
    ev_bev_row(bd, a0, a1, rd);
    ev_bev_row(bg, a0, a1, rg);
    const float inter = ev_clip_area(rg, rd);   // devRotateIoUEval(rbox1 = the query row = ground truth, rbox2 = detection)
    if (metric == 1) {
        const float area1 = rg[3] * rg[4], area2 = rd[3] * rd[4];
        out[p] = inter / (area1 + area2 - inter);
        return;
    }
    float v = inter;   // rinc; box3d_overlap_kernel(boxes = detections, qboxes = ground truths), criterion -1
    if (inter > 0) {
        const double min_z = fmin(bd[z_axis] + bd[z_axis + 3] * (1 - z_center), bg[z_axis] + bg[z_axis + 3] * (1 - z_center));
        const double max_z = fmax(bd[z_axis] - bd[z_axis + 3] * z_center, bg[z_axis] - bg[z_axis + 3] * z_center);
        const double iw = min_z - max_z;
        if (iw > 0) {
            const double area1 = bd[3] * bd[4] * bd[5], area2 = bg[3] * bg[4] * bg[5];
            const double inc = iw * (double)inter;
            v = (float)(inc / (area1 + area2 - inc));
        } else {
            v = 0.f;
        }
    }
    out[p] = v;
}

int ev_table(EvTable &tb, const int32_t *classes, int num_classes, const int32_t *difficulties, int num_difficulties, const double *min_overlaps,
             int num_overlaps, const char *who) {
    S2D_CHECK_ARG(classes && num_classes >= 1 && num_classes <= S2D_EVAL_MAX_CLASSES, "%s: %d classes (1..%d)", who, num_classes,
                  S2D_EVAL_MAX_CLASSES);
    S2D_CHECK_ARG(difficulties && num_difficulties >= 1 && num_difficulties <= 3, "%s: %d difficulties (1..3)", who, num_difficulties);
    S2D_CHECK_ARG(min_overlaps && num_overlaps >= 1 && num_overlaps <= 64, "%s: %d overlap values (1..64)", who, num_overlaps);
    for (int m = 0; m < num_classes; ++m) {
        S2D_CHECK_ARG(classes[m] >= 0 && classes[m] < S2D_EVAL_MAX_CLASSES, "%s: class %d (0..%d)", who, classes[m], S2D_EVAL_MAX_CLASSES - 1);
        tb.classes[m] = classes[m];
    }
    for (int l = 0; l < num_difficulties; ++l) {
        S2D_CHECK_ARG(difficulties[l] >= 0 && difficulties[l] <= 2, "%s: difficulty %d (0..2)", who, difficulties[l]);
        tb.diffs[l] = difficulties[l];
    }
    tb.num_classes = num_classes;
    tb.num_diffs = num_difficulties;
    tb.num_ov = num_overlaps;
    tb.min_ov = min_overlaps;
    return S2D_OK;
}

int ev_rows(EvRows &r, const float *overlaps, const double *det_img, const double *det_score, const int32_t *det_name, const double *gt_img,
            const double *gt_occ_trunc, const int32_t *gt_name, const int32_t *det_off, const int32_t *gt_off, const int64_t *ov_off, int frames,
            const char *who) {
    S2D_CHECK_ARG(frames >= 1 && det_off && gt_off && ov_off, "%s: %d frames (>= 1) with their row and pair offsets", who, frames);
    r = EvRows{overlaps, det_img, det_score, det_name, gt_img, gt_occ_trunc, gt_name, det_off, gt_off, ov_off};
    return S2D_OK;
}

}  // namespace
}  // namespace s2d

using namespace s2d;

extern "C" int s2d_eval_overlaps(int metric, const double *det_box, const double *det_img, const double *gt_box, const double *gt_img,
                                 const int32_t *det_off, const int32_t *gt_off, const int64_t *ov_off, int frames, int64_t pairs, int z_axis,
                                 double z_center, float *overlaps, s2d_stream_t stream) {
    S2D_CHECK_ARG(metric >= 0 && metric <= 2, "eval_overlaps: metric %d (0 bbox, 1 bev, 2 3d)", metric);
    S2D_CHECK_ARG(z_axis >= 0 && z_axis <= 2, "eval_overlaps: z_axis %d (0..2)", z_axis);
    S2D_CHECK_ARG(frames >= 1 && det_off && gt_off && ov_off, "eval_overlaps: %d frames (>= 1) with their row and pair offsets", frames);
    S2D_CHECK_ARG(pairs >= 0 && pairs <= (int64_t)INT_MAX * 256, "eval_overlaps: %lld pairs", (long long)pairs);
    if (pairs == 0) return S2D_OK;
    S2D_CHECK_ARG(det_box && det_img && gt_box && gt_img && overlaps, "eval_overlaps: null rows or output");
    hipLaunchKernelGGL(eval_overlaps_kernel, dim3((unsigned)ceil_div(pairs, 256)), dim3(256), 0, (hipStream_t)stream, metric, det_box, det_img,
                       gt_box, gt_img, det_off, gt_off, ov_off, frames, pairs, z_axis, z_center, overlaps);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_eval_match(const float *overlaps, const double *det_img, const double *det_score, const int32_t *det_name,
                              const double *gt_img, const double *gt_occ_trunc, const int32_t *gt_name, const int32_t *det_off,
                              const int32_t *gt_off, const int64_t *ov_off, int frames, const int32_t *classes, int num_classes,
                              const int32_t *difficulties, int num_difficulties, const double *min_overlaps, int num_overlaps, int64_t total_gt,
                              double *tp_scores, int32_t *counts, int64_t *pr, s2d_stream_t stream) {
    EvRows r;
    EvTable tb;
    int rc = ev_rows(r, overlaps, det_img, det_score, det_name, gt_img, gt_occ_trunc, gt_name, det_off, gt_off, ov_off, frames, "eval_match");
    if (rc != S2D_OK) return rc;
    rc = ev_table(tb, classes, num_classes, difficulties, num_difficulties, min_overlaps, num_overlaps, "eval_match");
    if (rc != S2D_OK) return rc;
    const int combos = num_classes * num_difficulties * num_overlaps;
    S2D_CHECK_ARG(combos <= 65535, "eval_match: %d (class, difficulty, overlap) combinations (at most 65535)", combos);
    S2D_CHECK_ARG(total_gt >= 0 && counts && pr && (total_gt == 0 || tp_scores), "eval_match: null output (or %lld ground-truth rows)",
                  (long long)total_gt);
    hipLaunchKernelGGL(eval_match_kernel, dim3(frames, combos), dim3(64), 0, (hipStream_t)stream, r, tb, total_gt, tp_scores, counts, pr,
                       combos * EV_PTS * 3);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_eval_pr(const float *overlaps, const double *det_img, const double *det_score, const int32_t *det_name, const double *gt_img,
                           const double *gt_occ_trunc, const int32_t *gt_name, const int32_t *det_off, const int32_t *gt_off,
                           const int64_t *ov_off, int frames, int metric, const int32_t *classes, int num_classes, const int32_t *difficulties,
                           int num_difficulties, const double *min_overlaps, int num_overlaps, const double *thresholds,
                           const int32_t *num_thresholds, int64_t *pr, s2d_stream_t stream) {
    EvRows r;
    EvTable tb;
    int rc = ev_rows(r, overlaps, det_img, det_score, det_name, gt_img, gt_occ_trunc, gt_name, det_off, gt_off, ov_off, frames, "eval_pr");
    if (rc != S2D_OK) return rc;
    rc = ev_table(tb, classes, num_classes, difficulties, num_difficulties, min_overlaps, num_overlaps, "eval_pr");
    if (rc != S2D_OK) return rc;
    const int combos = num_classes * num_difficulties * num_overlaps;
    S2D_CHECK_ARG(metric >= 0 && metric <= 2, "eval_pr: metric %d (0 bbox, 1 bev, 2 3d)", metric);
    S2D_CHECK_ARG(combos <= 65535, "eval_pr: %d (class, difficulty, overlap) combinations (at most 65535)", combos);
    S2D_CHECK_ARG(thresholds && num_thresholds && pr, "eval_pr: null thresholds or output");
    hipLaunchKernelGGL(eval_pr_kernel, dim3(frames, combos, EV_PTS), dim3(64), 0, (hipStream_t)stream, r, tb, metric, thresholds, num_thresholds,
                       pr);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
