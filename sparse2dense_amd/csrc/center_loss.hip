// CenterHead losses on the device maps, one pass per direction:
//   FastFocalLoss (/root/reference/det3d/models/losses/centernet_loss.py:33-54): on the clamped sigmoid map `out` [B,C,H,W]
//       neg = sum log(1-out) out^2 (1-target)^4 over every pixel,  pos = sum_m log(p_m) (1-p_m)^2 mask_m with p_m = out[b, cat_m, ind_m],
//       loss = -(pos + neg) / max(sum mask, 1)          (the reference's num_pos == 0 branch gives the same value)
//   RegLoss (centernet_loss.py:9-31): pred = out[b, :, ind_m]; loss_c = sum_{b,m} |pred*mask - target*mask| / (sum mask + 1e-4)
// composed from torch ops these are ~45 + ~20 launches of 3-5 us per step (permute / gather / pow / log / mul / sum chains and their
// backward); here 2 + 2 and 1 + 2.  Sums are folded in a fixed order; the backward's scatter uses atomicAdd only where two objects share
// a centre cell (as torch's gather backward does).
//
// Multi-task form (the six-task nuScenes head): s2d_center_tasks_loss_fwd / _bwd evaluate the same two losses for ALL tasks of a
// CenterHead from the hm LOGITS and the branch maps as the head produced them (reg[2] height[1] dim[3] (vel[2]) rot[2]: no torch.cat),
// in 2 launches forward and 1 zero-fill + 2 backward, whatever the number of tasks.  The per-task pointers travel as a kernel argument
// by value (CtTable), so nothing is copied to the device per step.  p = clamp(sigmoid(logit), 1e-4, 1 - 1e-4) is stored (the positives
// and preds["hm"] read it); the clamp's gradient follows torch (passes at the bounds inclusive, zero beyond).
#include "s2d_common.h"

namespace s2d {

constexpr int FOCAL_BLOCKS = 256;

__device__ __forceinline__ float block_sum_256(float v, float *sh) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wid] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void focal_neg_kernel(const float *__restrict__ out, const float *__restrict__ target, int64_t n,
                                                        float *__restrict__ partial) {
    __shared__ float sh[4];
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float p = out[i], t = 1.f - target[i];
        const float t2 = t * t;
        s += logf(1.f - p) * p * p * (t2 * t2);
    }
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one block: positives + fold of the negative partials.  res = {loss, pos, neg, num_pos}
__global__ __launch_bounds__(256) void focal_finalize_kernel(const float *__restrict__ out, const int64_t *__restrict__ ind, const uint8_t *__restrict__ mask,
                                                             const int64_t *__restrict__ cat, int batch, int classes, int64_t hw, int max_objs,
                                                             const float *__restrict__ partial, int n_partial, float *__restrict__ res) {
    __shared__ float sh[4];
    float pos = 0.f, cnt = 0.f, neg = 0.f;
    for (int i = threadIdx.x; i < batch * max_objs; i += 256) {
        if (!mask[i]) continue;
        const int b = i / max_objs;
        const float p = out[((int64_t)b * classes + cat[i]) * hw + ind[i]];
        pos += logf(p) * (1.f - p) * (1.f - p);
        cnt += 1.f;
    }
    for (int i = threadIdx.x; i < n_partial; i += 256) neg += partial[i];
    pos = block_sum_256(pos, sh);
    cnt = block_sum_256(cnt, sh);
    neg = block_sum_256(neg, sh);
    if (threadIdx.x == 0) {
        res[0] = -(pos + neg) / fmaxf(cnt, 1.f);
        res[1] = pos;
        res[2] = neg;
        res[3] = cnt;
    }
}

// d loss / d out over every pixel (negatives)
__global__ __launch_bounds__(256) void focal_bwd_neg_kernel(const float *__restrict__ out, const float *__restrict__ target, int64_t n,
                                                            const float *__restrict__ res, const float *__restrict__ go, float *__restrict__ dout) {
    const float coef = -go[0] / fmaxf(res[3], 1.f);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float p = out[i], t = 1.f - target[i];
        const float t2 = t * t, q = 1.f - p;
        dout[i] = coef * (t2 * t2) * (2.f * p * logf(q) - p * p / q);
    }
}

__global__ __launch_bounds__(256) void focal_bwd_pos_kernel(const float *__restrict__ out, const int64_t *__restrict__ ind, const uint8_t *__restrict__ mask,
                                                            const int64_t *__restrict__ cat, int batch, int classes, int64_t hw, int max_objs,
                                                            const float *__restrict__ res, const float *__restrict__ go, float *__restrict__ dout) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= batch * max_objs || !mask[i]) return;
    const int b = i / max_objs;
    const int64_t at = ((int64_t)b * classes + cat[i]) * hw + ind[i];
    const float p = out[at], q = 1.f - p;
    const float coef = -go[0] / fmaxf(res[3], 1.f);
    atomicAdd(dout + at, coef * (q * q / p - 2.f * q * logf(p)));
}

// res[c] = loss_c (c < channels), res[channels] = sum mask + 1e-4
__global__ __launch_bounds__(256) void regloss_fwd_kernel(const float *__restrict__ feat, const int64_t *__restrict__ ind, const uint8_t *__restrict__ mask,
                                                          const float *__restrict__ target, int batch, int channels, int64_t hw, int max_objs,
                                                          float *__restrict__ res) {
    __shared__ float sh[4];
    float cnt = 0.f;
    for (int i = threadIdx.x; i < batch * max_objs; i += 256) cnt += mask[i] ? 1.f : 0.f;
    cnt = block_sum_256(cnt, sh) + 1e-4f;
    for (int c = 0; c < channels; ++c) {
        float s = 0.f;
        for (int i = threadIdx.x; i < batch * max_objs; i += 256) {
            if (!mask[i]) continue;
            const int b = i / max_objs;
            s += fabsf(feat[((int64_t)b * channels + c) * hw + ind[i]] - target[(int64_t)i * channels + c]);
        }
        s = block_sum_256(s, sh);
        if (threadIdx.x == 0) res[c] = s / cnt;
    }
    if (threadIdx.x == 0) res[channels] = cnt;
}

__global__ __launch_bounds__(256) void regloss_bwd_kernel(const float *__restrict__ feat, const int64_t *__restrict__ ind, const uint8_t *__restrict__ mask,
                                                          const float *__restrict__ target, int batch, int channels, int64_t hw, int max_objs,
                                                          const float *__restrict__ res, const float *__restrict__ go, float *__restrict__ dfeat) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= batch * max_objs * channels) return;
    const int c = t % channels, i = t / channels;
    if (!mask[i]) return;
    const int b = i / max_objs;
    const int64_t at = ((int64_t)b * channels + c) * hw + ind[i];
    const float d = feat[at] - target[(int64_t)i * channels + c];
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    atomicAdd(dfeat + at, go[c] * sgn / res[channels]);
}

// ---- all tasks of a CenterHead in one node ---------------------------------------------------------------------------------------
constexpr int CT_MAX_TASKS = 8;
constexpr int CT_BLOCKS = 64;      // negative-term partials per task
constexpr int CT_RES = 16;         // floats per result row: loss, hm_loss, loc_loss, loc_loss_elem[10], num_positive, (2 unused)
constexpr float CT_LO = 1e-4f, CT_HI = (float)(1 - 1e-4);

struct CtTable {
    s2d_center_task t[CT_MAX_TASKS];
};

__device__ __forceinline__ float ct_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// channel c of the regression vector: its map element at (b, cell) and its target column
__device__ __forceinline__ int64_t ct_channel(const s2d_center_task &t, int c, int b, int64_t hw, int64_t cell, const float **map, float **dmap,
                                              int *tcol) {
    const bool vel = t.vel != nullptr;
    int cc, n;
    if (c < 2) { *map = t.reg; *dmap = t.d_reg; cc = c; n = 2; }
    else if (c == 2) { *map = t.height; *dmap = t.d_height; cc = 0; n = 1; }
    else if (c < 6) { *map = t.dim; *dmap = t.d_dim; cc = c - 3; n = 3; }
    else if (vel && c < 8) { *map = t.vel; *dmap = t.d_vel; cc = c - 6; n = 2; }
    else { *map = t.rot; *dmap = t.d_rot; cc = c - (vel ? 8 : 6); n = 2; }
    *tcol = vel || c < 6 ? c : c + 2;   // without a velocity branch the target columns are [0..5, 8, 9]
    return ((int64_t)b * n + cc) * hw + cell;
}

// grid (blocks, tasks): p = clamp(sigmoid(logit)) stored, negative-term partial per block
__global__ __launch_bounds__(256) void center_tasks_neg_kernel(CtTable tb, int batch, int64_t hw, float *__restrict__ partial) {
    __shared__ float sh[4];
    const s2d_center_task &t = tb.t[blockIdx.y];
    const int64_t n = (int64_t)batch * t.classes * hw;
    const float *__restrict__ logit = t.hm_logit, *__restrict__ target = t.hm;
    float *__restrict__ prob = t.p;
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float p = fminf(fmaxf(ct_sigmoid(logit[i]), CT_LO), CT_HI), u = 1.f - target[i];
        const float u2 = u * u;
        prob[i] = p;
        s += logf(1.f - p) * p * p * (u2 * u2);
    }
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// one block per task: positives, fold of the partials, per-channel L1 sums gathered from the branch maps, sum(mask)
__global__ __launch_bounds__(256) void center_tasks_finalize_kernel(CtTable tb, int batch, int64_t hw, int max_objs, int channels,
                                                                    const float *__restrict__ code_weights, float weight,
                                                                    const float *__restrict__ partial, int n_partial, float *__restrict__ loss,
                                                                    float *__restrict__ loc_loss, float *__restrict__ res) {
    __shared__ float sh[4];
    const s2d_center_task &t = tb.t[blockIdx.x];
    float pos = 0.f, cnt = 0.f, neg = 0.f, l1[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < batch * max_objs; i += 256) {
        if (!t.mask[i]) continue;
        const int b = i / max_objs;
        const int64_t cell = t.ind[i];
        const float p = t.p[((int64_t)b * t.classes + t.cat[i]) * hw + cell];
        pos += logf(p) * (1.f - p) * (1.f - p);
        cnt += 1.f;
#pragma unroll
        for (int c = 0; c < 10; ++c)
            if (c < channels) {
                const float *map;
                float *dmap;
                int tcol;
                const int64_t at = ct_channel(t, c, b, hw, cell, &map, &dmap, &tcol);
                l1[c] += fabsf(map[at] - t.anno_box[(int64_t)i * 10 + tcol]);
            }
    }
    for (int i = threadIdx.x; i < n_partial; i += 256) neg += partial[blockIdx.x * n_partial + i];
    pos = block_sum_256(pos, sh);
    cnt = block_sum_256(cnt, sh);
    neg = block_sum_256(neg, sh);
    float loc = 0.f;
    float *row = res + blockIdx.x * CT_RES;
#pragma unroll
    for (int c = 0; c < 10; ++c) {
        const float v = c < channels ? block_sum_256(l1[c], sh) / (cnt + 1e-4f) : 0.f;   // (channels is uniform: every thread takes the barrier)
        if (c < channels) loc += v * code_weights[c];
        if (threadIdx.x == 0) row[3 + c] = v;
    }
    if (threadIdx.x == 0) {
        const float hm_loss = -(pos + neg) / fmaxf(cnt, 1.f);
        row[0] = loss[blockIdx.x] = hm_loss + weight * loc;
        row[1] = hm_loss;
        row[2] = loc_loss[blockIdx.x] = loc;
        row[13] = cnt;
        row[14] = row[15] = 0.f;
    }
}

// upstream factors of task t: the heat-map term takes go_loss, the regression term go_loss * weight + go_loc (either may be absent)
__device__ __forceinline__ void ct_upstream(const float *go_loss, const float *go_loc, int t, float weight, float *g_hm, float *g_loc) {
    const float gl = go_loss ? go_loss[t] : 0.f;
    *g_hm = gl;
    *g_loc = gl * weight + (go_loc ? go_loc[t] : 0.f);
}

// grid (blocks, tasks): d logit of the negative term at every pixel
__global__ __launch_bounds__(256) void center_tasks_bwd_dense_kernel(CtTable tb, int batch, int64_t hw, const float *__restrict__ res,
                                                                     const float *__restrict__ go_loss, const float *__restrict__ go_loc, float weight) {
    const s2d_center_task &t = tb.t[blockIdx.y];
    float g_hm, g_loc;
    ct_upstream(go_loss, go_loc, blockIdx.y, weight, &g_hm, &g_loc);
    const float coef = -g_hm / fmaxf(res[blockIdx.y * CT_RES + 13], 1.f);
    const int64_t n = (int64_t)batch * t.classes * hw;
    const float *__restrict__ logit = t.hm_logit, *__restrict__ target = t.hm;
    float *__restrict__ dlogit = t.d_logit;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float p = ct_sigmoid(logit[i]), u = 1.f - target[i];
        const float u2 = u * u, q = 1.f - p;
        const bool pass = p >= CT_LO && p <= CT_HI;   // torch.clamp's backward: the bounds pass
        dlogit[i] = pass ? coef * (u2 * u2) * (2.f * p * logf(q) - p * p / q) * (p * q) : 0.f;
    }
}

// grid (blocks, tasks), one thread per object slot: positive term into d logit, the regression scatter into the branch gradients
__global__ __launch_bounds__(256) void center_tasks_bwd_obj_kernel(CtTable tb, int batch, int64_t hw, int max_objs, int channels,
                                                                   const float *__restrict__ code_weights, float weight, const float *__restrict__ res,
                                                                   const float *__restrict__ go_loss, const float *__restrict__ go_loc) {
    const s2d_center_task &t = tb.t[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= batch * max_objs || !t.mask[i]) return;
    float g_hm, g_loc;
    ct_upstream(go_loss, go_loc, blockIdx.y, weight, &g_hm, &g_loc);
    const float cnt = res[blockIdx.y * CT_RES + 13];
    const int b = i / max_objs;
    const int64_t cell = t.ind[i];
    const int64_t at = ((int64_t)b * t.classes + t.cat[i]) * hw + cell;
    const float s = ct_sigmoid(t.hm_logit[at]);
    if (s >= CT_LO && s <= CT_HI) {
        const float q = 1.f - s;
        atomicAdd(t.d_logit + at, -g_hm / fmaxf(cnt, 1.f) * (q * q / s - 2.f * q * logf(s)) * (s * q));
    }
    const float scale = g_loc / (cnt + 1e-4f);
    for (int c = 0; c < channels; ++c) {
        const float *map;
        float *dmap;
        int tcol;
        const int64_t a = ct_channel(t, c, b, hw, cell, &map, &dmap, &tcol);
        const float d = map[a] - t.anno_box[(int64_t)i * 10 + tcol];
        const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        if (sgn != 0.f) atomicAdd(dmap + a, scale * code_weights[c] * sgn);
    }
}

static int ct_check_table(const s2d_center_task *tasks, int num_tasks, int batch, int64_t hw, int max_objs, bool bwd, CtTable *tb, int *channels,
                          int64_t *max_n) {
    S2D_CHECK_ARG(tasks && num_tasks > 0 && num_tasks <= CT_MAX_TASKS, "center_tasks_loss: 1..%d tasks expected", CT_MAX_TASKS);
    S2D_CHECK_ARG(batch > 0 && hw > 0 && max_objs > 0 && (int64_t)batch * max_objs < (1ll << 31), "center_tasks_loss: bad sizes");
    memset(tb, 0, sizeof(*tb));
    *max_n = 0;
    for (int i = 0; i < num_tasks; ++i) {
        const s2d_center_task &t = tasks[i];
        S2D_CHECK_ARG(t.classes > 0 && t.hm_logit && t.reg && t.height && t.dim && t.rot && t.hm && t.ind && t.mask && t.cat && t.anno_box && t.p,
                      "center_tasks_loss: task %d has a null map or target", i);
        S2D_CHECK_ARG((t.vel != nullptr) == (tasks[0].vel != nullptr), "center_tasks_loss: either every task has a vel branch or none");
        if (bwd)
            S2D_CHECK_ARG(t.d_logit && t.d_reg && t.d_height && t.d_dim && t.d_rot && (t.d_vel != nullptr) == (t.vel != nullptr),
                          "center_tasks_loss_bwd: task %d has a null gradient map", i);
        tb->t[i] = t;
        *max_n = std::max<int64_t>(*max_n, (int64_t)batch * t.classes * hw);
    }
    *channels = tasks[0].vel ? 10 : 8;
    return S2D_OK;
}

}  // namespace s2d

using namespace s2d;

extern "C" size_t s2d_focal_workspace_bytes(void) { return (size_t)FOCAL_BLOCKS * sizeof(float) + 256; }

/* out / target: fp32 [batch][classes][hw] contiguous; ind, cat: int64 [batch][max_objs]; mask: uint8 [batch][max_objs];
 * res (device, 4 floats): loss, positive sum, negative sum, number of positives */
extern "C" int s2d_focal_fwd(const float *out, const float *target, const int64_t *ind, const uint8_t *mask, const int64_t *cat, int batch,
                             int classes, int64_t hw, int max_objs, float *res, void *ws, size_t ws_bytes, s2d_stream_t stream) {
    S2D_CHECK_ARG(out && target && ind && mask && cat && res && batch > 0 && classes > 0 && hw > 0 && max_objs > 0, "focal_fwd: bad argument");
    if (!ws || ws_bytes < s2d_focal_workspace_bytes()) {
        set_error("focal_fwd: workspace too small");
        return S2D_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)batch * classes * hw;
    const int nb = (int)std::min<int64_t>(FOCAL_BLOCKS, ceil_div(n, 256));
    hipLaunchKernelGGL(focal_neg_kernel, dim3(nb), dim3(256), 0, st, out, target, n, (float *)ws);
    hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(256), 0, st, out, ind, mask, cat, batch, classes, hw, max_objs, (const float *)ws, nb,
                       res);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

/* dout (fp32, same shape as out) = go[0] * d loss / d out; res = the forward's result vector */
extern "C" int s2d_focal_bwd(const float *out, const float *target, const int64_t *ind, const uint8_t *mask, const int64_t *cat, int batch,
                             int classes, int64_t hw, int max_objs, const float *res, const float *go, float *dout, s2d_stream_t stream) {
    S2D_CHECK_ARG(out && target && ind && mask && cat && res && go && dout && batch > 0 && classes > 0 && hw > 0 && max_objs > 0,
                  "focal_bwd: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)batch * classes * hw;
    hipLaunchKernelGGL(focal_bwd_neg_kernel, dim3((unsigned)std::min<int64_t>(2048, ceil_div(n, 256))), dim3(256), 0, st, out, target, n, res, go,
                       dout);
    hipLaunchKernelGGL(focal_bwd_pos_kernel, dim3((unsigned)ceil_div(batch * max_objs, 256)), dim3(256), 0, st, out, ind, mask, cat, batch, classes,
                       hw, max_objs, res, go, dout);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

/* feat: fp32 [batch][channels][hw]; target: fp32 [batch][max_objs][channels]; res (device, channels + 1 floats): the per-channel
 * losses, then the denominator sum(mask) + 1e-4 */
extern "C" int s2d_regloss_fwd(const float *feat, const int64_t *ind, const uint8_t *mask, const float *target, int batch, int channels,
                               int64_t hw, int max_objs, float *res, s2d_stream_t stream) {
    S2D_CHECK_ARG(feat && ind && mask && target && res && batch > 0 && channels > 0 && hw > 0 && max_objs > 0, "regloss_fwd: bad argument");
    hipLaunchKernelGGL(regloss_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, feat, ind, mask, target, batch, channels, hw, max_objs, res);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

/* dfeat (fp32, zero-filled here) = sum_c go[c] * d loss_c / d feat */
extern "C" int s2d_regloss_bwd(const float *feat, const int64_t *ind, const uint8_t *mask, const float *target, int batch, int channels,
                               int64_t hw, int max_objs, const float *res, const float *go, float *dfeat, s2d_stream_t stream) {
    S2D_CHECK_ARG(feat && ind && mask && target && res && go && dfeat && batch > 0 && channels > 0 && hw > 0 && max_objs > 0,
                  "regloss_bwd: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = zero_async(dfeat, (size_t)batch * channels * hw * sizeof(float), st)) return rc;   // (a kernel, not a memset node: see zero_async)
    hipLaunchKernelGGL(regloss_bwd_kernel, dim3((unsigned)ceil_div(batch * max_objs * channels, 256)), dim3(256), 0, st, feat, ind, mask, target,
                       batch, channels, hw, max_objs, res, go, dfeat);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" size_t s2d_center_tasks_loss_workspace_bytes(void) { return (size_t)CT_MAX_TASKS * CT_BLOCKS * sizeof(float) + 256; }

/* All tasks of a CenterHead at once.  tasks: HOST array (copied into the kernel arguments).  code_weights: device, 10 floats with a vel
 * branch, else 8.  loss / loc_loss: device [num_tasks]; res: device [num_tasks][16] = loss, hm_loss, loc_loss, loc_loss_elem[10],
 * num_positive, 0, 0.  Writes every task's p map. */
extern "C" int s2d_center_tasks_loss_fwd(const s2d_center_task *tasks, int num_tasks, int batch, int64_t hw, int max_objs,
                                         const float *code_weights, float weight, float *loss, float *loc_loss, float *res, void *ws,
                                         size_t ws_bytes, s2d_stream_t stream) {
    CtTable tb;
    int channels;
    int64_t max_n;
    if (int rc = ct_check_table(tasks, num_tasks, batch, hw, max_objs, false, &tb, &channels, &max_n)) return rc;
    S2D_CHECK_ARG(code_weights && loss && loc_loss && res, "center_tasks_loss_fwd: null argument");
    if (!ws || ws_bytes < s2d_center_tasks_loss_workspace_bytes()) {
        set_error("center_tasks_loss_fwd: workspace too small");
        return S2D_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)std::min<int64_t>(CT_BLOCKS, ceil_div(max_n, 256));
    hipLaunchKernelGGL(center_tasks_neg_kernel, dim3(nb, num_tasks), dim3(256), 0, st, tb, batch, hw, (float *)ws);
    hipLaunchKernelGGL(center_tasks_finalize_kernel, dim3(num_tasks), dim3(256), 0, st, tb, batch, hw, max_objs, channels, code_weights, weight,
                       (const float *)ws, nb, loss, loc_loss, res);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

/* d_logit of every task is fully written; the branch gradients (d_reg ... d_rot of every task) must lie inside [dbranch, dbranch +
 * dbranch_bytes), which is zero-filled here (a kernel, not a memset node) before the scatter.  go_loss / go_loc: device [num_tasks],
 * the upstream gradients of loss and of loc_loss (either may be NULL = zero). */
extern "C" int s2d_center_tasks_loss_bwd(const s2d_center_task *tasks, int num_tasks, int batch, int64_t hw, int max_objs,
                                         const float *code_weights, float weight, const float *res, const float *go_loss, const float *go_loc,
                                         void *dbranch, size_t dbranch_bytes, s2d_stream_t stream) {
    CtTable tb;
    int channels;
    int64_t max_n;
    if (int rc = ct_check_table(tasks, num_tasks, batch, hw, max_objs, true, &tb, &channels, &max_n)) return rc;
    S2D_CHECK_ARG(code_weights && res && dbranch && (go_loss || go_loc), "center_tasks_loss_bwd: null argument");
    for (int i = 0; i < num_tasks; ++i) {
        const s2d_center_task &t = tasks[i];
        const struct { const float *p; int n; } maps[5] = {{t.d_reg, 2}, {t.d_height, 1}, {t.d_dim, 3}, {t.d_vel, 2}, {t.d_rot, 2}};
        for (const auto &m : maps)
            S2D_CHECK_ARG(!m.p || ((const char *)m.p >= (const char *)dbranch &&
                                   (const char *)(m.p + (int64_t)batch * m.n * hw) <= (const char *)dbranch + dbranch_bytes),
                          "center_tasks_loss_bwd: a branch gradient of task %d lies outside the zero-filled buffer", i);
    }
    hipStream_t st = (hipStream_t)stream;
    if (int rc = zero_async(dbranch, dbranch_bytes, st)) return rc;
    hipLaunchKernelGGL(center_tasks_bwd_dense_kernel, dim3((unsigned)std::min<int64_t>(256, ceil_div(max_n, 256)), num_tasks), dim3(256), 0, st, tb,
                       batch, hw, res, go_loss, go_loc, weight);
    hipLaunchKernelGGL(center_tasks_bwd_obj_kernel, dim3((unsigned)ceil_div((int64_t)batch * max_objs, 256), num_tasks), dim3(256), 0, st, tb, batch,
                       hw, max_objs, channels, code_weights, weight, res, go_loss, go_loc);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
