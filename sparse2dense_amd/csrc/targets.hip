// CenterPoint training targets on the device: AssignLabel.__call__ for the one-task Waymo head
// (/root/reference/det3d/datasets/pipelines/preprocess.py:489-653) with gaussian_radius / gaussian2D / draw_umich_gaussian of
// /root/reference/det3d/core/utils/center_utils.py:18-64 and box_np_ops.limit_period (det3d/core/bbox/box_np_ops.py:360-361).
// In the reference this is per-frame numpy in the DataLoader workers; at hundreds of frames/s per GPU the targets have to be
// produced where the frames already are.
//
// One thread per (frame, object slot k < max_objs):
//   yaw <- yaw - floor(yaw / 2pi + 0.5) * 2pi                                              (fp32, as numpy on the fp32 box array)
//   w, l in feature-map cells (fp32); radius = max(min_radius, int(gaussian_radius((l, w), overlap)))   (float64 roots)
//   ct = ((x - x0) / vx / f, (y - y0) / vy / f) fp32; ct_int = trunc(ct); skipped when outside the map
//   hm[cls] = max(hm[cls], gaussian)  on the (2r+1)^2 window clipped to the map        (float atomicMax: order independent)
//   ind = y*W + x, mask = 1, cat = cls, anno_box = (ct - ct_int, z, log(w,l,h), vx, vy, sin yaw, cos yaw)
//   gt_boxes_and_cls[k] = (x, y, z, w, l, h, yaw, vx, vy, class)                          (two-stage code, preprocess.py:626-649)
// Boxes are [frames][max_boxes][9] = (x,y,z,w,l,h,vx,vy,yaw) fp32, classes int32 (1-based; <= 0 = padding).  hm must be zeroed
// by the caller (the other outputs are fully written).
// assign_label_tasks_kernel does the same for a table of tasks from boxes in their ORIGINAL order (the regrouping per task and class
// happens on the device): see the comment in front of it.
#include "s2d_common.h"

namespace s2d {

struct TgtGeo {
    float x0, y0, vx, vy;
    int factor, fw, fh, num_classes, max_objs, min_radius;
    double overlap;
};

__device__ __forceinline__ double tgt_gaussian_radius(double height, double width, double mo) {
    const double b1 = height + width, c1 = width * height * (1 - mo) / (1 + mo);
    const double r1 = (b1 + sqrt(b1 * b1 - 4 * c1)) / 2;
    const double b2 = 2 * (height + width), c2 = (1 - mo) * width * height;
    const double r2 = (b2 + sqrt(b2 * b2 - 16 * c2)) / 2;
    const double a3 = 4 * mo, b3 = -2 * mo * (height + width), c3 = (mo - 1) * width * height;
    const double r3 = (b3 + sqrt(b3 * b3 - 4 * a3 * c3)) / 2;
    return fmin(r1, fmin(r2, r3));
}

// One object of class `cls` (1-based inside its plane group `planes`, which holds the heat-map planes of the object's task in this frame):
// the blob, and the slot's values.  Returns false (and leaves the outputs alone) for a degenerate or out-of-map box.
__device__ __forceinline__ bool tgt_object(const float *__restrict__ bx, float yaw, int cls, const TgtGeo &g, float *__restrict__ planes, float *ab,
                                           int64_t *o_ind) {
    const float w = bx[3] / g.vx / (float)g.factor, l = bx[4] / g.vy / (float)g.factor;
    if (!(w > 0.f && l > 0.f)) return false;
    int radius = (int)tgt_gaussian_radius((double)l, (double)w, g.overlap);
    radius = radius > g.min_radius ? radius : g.min_radius;
    const float cx = (bx[0] - g.x0) / g.vx / (float)g.factor, cy = (bx[1] - g.y0) / g.vy / (float)g.factor;
    const int xi = (int)cx, yi = (int)cy;   // truncation, as ndarray.astype(int32)
    if (!(xi >= 0 && xi < g.fw && yi >= 0 && yi < g.fh)) return false;
    const double sigma = (2 * radius + 1) / 6.0;
    const int left = min(xi, radius), right = min(g.fw - xi, radius + 1);
    const int top = min(yi, radius), bottom = min(g.fh - yi, radius + 1);
    float *plane = planes + (int64_t)(cls - 1) * g.fh * g.fw;
    for (int dy = -top; dy < bottom; ++dy)
        for (int dx = -left; dx < right; ++dx) {
            const double gv = exp(-(double)(dx * dx + dy * dy) / (2 * sigma * sigma));
            const float gf = gv < 2.220446049250313e-16 ? 0.f : (float)gv;
            // non-negative floats order like their bit patterns
            atomicMax(reinterpret_cast<int *>(plane + (int64_t)(yi + dy) * g.fw + xi + dx), __float_as_int(gf));
        }
    *o_ind = (int64_t)yi * g.fw + xi;
    ab[0] = cx - (float)xi; ab[1] = cy - (float)yi; ab[2] = bx[2];
    ab[3] = logf(bx[3]); ab[4] = logf(bx[4]); ab[5] = logf(bx[5]);
    ab[6] = bx[6]; ab[7] = bx[7]; ab[8] = sinf(yaw); ab[9] = cosf(yaw);
    return true;
}

__global__ __launch_bounds__(256) void assign_label_kernel(const float *__restrict__ boxes, const int32_t *__restrict__ classes, int frames, int max_boxes,
                                                           TgtGeo g, float *__restrict__ hm, float *__restrict__ anno_box, int64_t *__restrict__ ind,
                                                           uint8_t *__restrict__ mask, int64_t *__restrict__ cat, float *__restrict__ boxes_cls) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= frames * g.max_objs) return;
    const int b = i / g.max_objs, k = i - b * g.max_objs;
    float ab[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, bc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int64_t o_ind = 0, o_cat = 0;
    uint8_t o_mask = 0;
    if (k < max_boxes) {
        const float *bx = boxes + ((int64_t)b * max_boxes + k) * 9;
        const int cls = classes[(int64_t)b * max_boxes + k];
        if (cls > 0 && cls <= g.num_classes) {
            const float two_pi = (float)(3.141592653589793 * 2);
            const float yaw = bx[8] - floorf(bx[8] / two_pi + 0.5f) * two_pi;
            bc[0] = bx[0]; bc[1] = bx[1]; bc[2] = bx[2]; bc[3] = bx[3]; bc[4] = bx[4]; bc[5] = bx[5];
            bc[6] = yaw; bc[7] = bx[6]; bc[8] = bx[7]; bc[9] = (float)cls;
            if (tgt_object(bx, yaw, cls, g, hm + (int64_t)b * g.num_classes * g.fh * g.fw, ab, &o_ind)) {
                o_cat = cls - 1;
                o_mask = 1;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 10; ++e) {
        anno_box[(int64_t)i * 10 + e] = ab[e];
        if (boxes_cls) boxes_cls[(int64_t)i * 10 + e] = bc[e];
    }
    ind[i] = o_ind;
    mask[i] = o_mask;
    cat[i] = o_cat;
}

// The same for a table of tasks (the nuScenes configs: six tasks over ten classes), one workgroup per frame.  The reference regroups the
// frame's boxes per task and class by class inside a task (np.where per class, concatenated: preprocess.py:506-534), so slot k of task t
// is the k-th object in (class, original index) order among the task's objects, and row r of gt_boxes_and_cls is the r-th object in
// that order over all tasks (tasks own consecutive class ranges, so the flattened order is the global (class, index) order).  Each
// thread ranks its object against the frame's classes, staged through LDS 256 at a time; objects whose slot is >= max_objs are dropped
// entirely (num_objs = min(len, max_objs), :569).  A degenerate or out-of-map box keeps its slot with mask 0 and a zero row (new_idx = k).
// Per task the outputs are laid out task after task: hm [frames][n_t][fh][fw] at plane offset frames * off_t, the slot arrays
// [tasks][frames][max_objs](x10).  Everything but hm is written here (zero rows first, then the objects, ordered by the barrier); hm
// must be zeroed by the caller.
constexpr int TGT_MAX_TASKS = 8;
struct TgtTasks {
    int n;
    int off[TGT_MAX_TASKS + 1];   // task t owns the global classes off[t]+1 .. off[t+1]
};

__global__ __launch_bounds__(256) void assign_label_tasks_kernel(const float *__restrict__ boxes, const int32_t *__restrict__ classes, int frames,
                                                                 int max_boxes, TgtGeo g, TgtTasks tk, float *__restrict__ hm,
                                                                 float *__restrict__ anno_box, int64_t *__restrict__ ind, uint8_t *__restrict__ mask,
                                                                 int64_t *__restrict__ cat, float *__restrict__ boxes_cls) {
    __shared__ int sh_cls[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int last_cls = tk.off[tk.n];
    for (int t = 0; t < tk.n; ++t) {
        const int64_t row0 = ((int64_t)t * frames + b) * g.max_objs;
        for (int k = tid; k < g.max_objs; k += 256) {
            ind[row0 + k] = 0;
            mask[row0 + k] = 0;
            cat[row0 + k] = 0;
        }
        for (int e = tid; e < g.max_objs * 10; e += 256) anno_box[row0 * 10 + e] = 0.f;
    }
    if (boxes_cls)
        for (int e = tid; e < g.max_objs * 10; e += 256) boxes_cls[(int64_t)b * g.max_objs * 10 + e] = 0.f;
    __syncthreads();   // (also orders the zero rows in global memory before this workgroup's object rows)
    const int32_t *cl = classes + (int64_t)b * max_boxes;
    for (int base = 0; base < max_boxes; base += 256) {
        const int i = base + tid;
        int ci = 0, lo = 0, task = 0;
        if (i < max_boxes) {
            const int c = cl[i];
            if (c > 0 && c <= last_cls) ci = c;
        }
        if (ci)
            for (int t = 0; t < tk.n; ++t)
                if (ci > tk.off[t] && ci <= tk.off[t + 1]) {
                    task = t;
                    lo = tk.off[t];
                }
        int slot = 0, flat = 0;
        for (int jb = 0; jb < max_boxes; jb += 256) {
            __syncthreads();
            const int j = jb + tid;
            int cj = 0;
            if (j < max_boxes) {
                cj = cl[j];
                if (cj <= 0 || cj > last_cls) cj = 0;
            }
            sh_cls[tid] = cj;
            __syncthreads();
            if (ci) {
                const int n = min(256, max_boxes - jb);
                for (int jj = 0; jj < n; ++jj) {
                    const int c = sh_cls[jj];
                    if (c != 0 && (c < ci || (c == ci && jb + jj < i))) {
                        ++flat;
                        slot += c > lo ? 1 : 0;   // lo < c <= ci: the same task
                    }
                }
            }
        }
        if (!ci) continue;
        const float *bx = boxes + ((int64_t)b * max_boxes + i) * 9;
        const float two_pi = (float)(3.141592653589793 * 2);
        const float yaw = bx[8] - floorf(bx[8] / two_pi + 0.5f) * two_pi;
        if (boxes_cls && flat < g.max_objs) {
            float *bc = boxes_cls + ((int64_t)b * g.max_objs + flat) * 10;
            bc[0] = bx[0]; bc[1] = bx[1]; bc[2] = bx[2]; bc[3] = bx[3]; bc[4] = bx[4]; bc[5] = bx[5];
            bc[6] = yaw; bc[7] = bx[6]; bc[8] = bx[7]; bc[9] = (float)ci;
        }
        if (slot >= g.max_objs) continue;
        const int n_t = tk.off[task + 1] - lo;
        float ab[10];
        int64_t o_ind;
        if (!tgt_object(bx, yaw, ci - lo, g, hm + ((int64_t)frames * lo + (int64_t)b * n_t) * g.fh * g.fw, ab, &o_ind)) continue;
        const int64_t row = ((int64_t)task * frames + b) * g.max_objs + slot;
#pragma unroll
        for (int e = 0; e < 10; ++e) anno_box[row * 10 + e] = ab[e];
        ind[row] = o_ind;
        mask[row] = 1;
        cat[row] = ci - lo - 1;
    }
}

}  // namespace s2d

using namespace s2d;

extern "C" int s2d_assign_label(const float *gt_boxes, const int32_t *gt_classes, int frames, int max_boxes, const float pc_range_xy[2],
                                const float voxel_size_xy[2], int out_size_factor, int fmap_w, int fmap_h, int num_classes, int max_objs,
                                double gaussian_overlap, int min_radius, float *hm_zeroed, float *anno_box, int64_t *ind, uint8_t *mask,
                                int64_t *cat, float *gt_boxes_and_cls, s2d_stream_t stream) {
    S2D_CHECK_ARG(frames > 0 && max_boxes >= 0 && max_objs > 0 && fmap_w > 0 && fmap_h > 0 && num_classes > 0 && out_size_factor > 0,
                  "assign_label: bad sizes");
    S2D_CHECK_ARG(pc_range_xy && voxel_size_xy && hm_zeroed && anno_box && ind && mask && cat && (max_boxes == 0 || (gt_boxes && gt_classes)),
                  "assign_label: null argument");
    TgtGeo g{pc_range_xy[0], pc_range_xy[1], voxel_size_xy[0], voxel_size_xy[1], out_size_factor, fmap_w, fmap_h, num_classes, max_objs,
             min_radius, gaussian_overlap};
    const int total = frames * max_objs;
    hipLaunchKernelGGL(assign_label_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, gt_boxes, gt_classes, frames, max_boxes,
                       g, hm_zeroed, anno_box, ind, mask, cat, gt_boxes_and_cls);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_assign_label_tasks(const float *gt_boxes, const int32_t *gt_classes, int frames, int max_boxes, const int32_t *task_num_classes,
                                      int num_tasks, const float pc_range_xy[2], const float voxel_size_xy[2], int out_size_factor, int fmap_w,
                                      int fmap_h, int max_objs, double gaussian_overlap, int min_radius, float *hm_zeroed, float *anno_box,
                                      int64_t *ind, uint8_t *mask, int64_t *cat, float *gt_boxes_and_cls, s2d_stream_t stream) {
    S2D_CHECK_ARG(frames > 0 && max_boxes >= 0 && max_objs > 0 && fmap_w > 0 && fmap_h > 0 && out_size_factor > 0, "assign_label_tasks: bad sizes");
    S2D_CHECK_ARG(task_num_classes && num_tasks > 0 && num_tasks <= TGT_MAX_TASKS, "assign_label_tasks: 1..%d tasks expected", TGT_MAX_TASKS);
    S2D_CHECK_ARG(pc_range_xy && voxel_size_xy && hm_zeroed && anno_box && ind && mask && cat && (max_boxes == 0 || (gt_boxes && gt_classes)),
                  "assign_label_tasks: null argument");
    TgtTasks tk{};
    tk.n = num_tasks;
    for (int t = 0; t < num_tasks; ++t) {
        S2D_CHECK_ARG(task_num_classes[t] > 0, "assign_label_tasks: task %d has no class", t);
        tk.off[t + 1] = tk.off[t] + task_num_classes[t];
    }
    TgtGeo g{pc_range_xy[0], pc_range_xy[1], voxel_size_xy[0], voxel_size_xy[1], out_size_factor, fmap_w, fmap_h, tk.off[num_tasks], max_objs,
             min_radius, gaussian_overlap};
    hipLaunchKernelGGL(assign_label_tasks_kernel, dim3(frames), dim3(256), 0, (hipStream_t)stream, gt_boxes, gt_classes, frames, max_boxes, g, tk,
                       hm_zeroed, anno_box, ind, mask, cat, gt_boxes_and_cls);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
