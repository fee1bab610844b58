// The TRAINING branch of the RoI MLP of the two-stage head on the device: forward with batch statistics and dropout masks, the two RoI
// losses, and the backward of all of it (roi_head.py:70-106, roi_head_template.py:94-151 of the reference; the eval branch is
// csrc/roi_mlp.hip, whose layer table - s2d_roi_mlp_plan - and packed B-fragment image the forward products reuse).
//
// A hidden layer is z = a . W^T, y = gamma * (z - mean) * invstd + beta with the batch mean and biased variance over the R rows,
// a' = relu(y) * mask * keep_scale.  A batch norm couples all rows, so a layer can only start when the layer before it has finished on the
// whole grid: ONE LAUNCH PER DEPTH, the two branches' layers of equal depth in one launch (blockIdx.y), no cooperative launch, no spin.
//
// Forward launch of a layer (a workgroup = 16 rows, 4 waves, v_mfma_f32_16x16x4_f32 as in the eval kernel):
//   prologue  merge the producer's per-tile (mean, M2) in tile order with Chan's formula (counts are 16, the last tile's is ragged) - the
//             variance is never formed as E[z^2] - E[z]^2; norm + ReLU + mask are applied while the A tile is staged into LDS; rows past R
//             are forced to zero AFTER the transform.  One designated workgroup (tile 0 of the first consumer) also stores (mean, invstd)
//             for the backward and moves the running statistics (momentum, unbiased variance).
//   product   A from LDS, B from the packed image; a first layer wider than 256 channels is staged in chunks of 256.
//   epilogue  z [R][cout] and the tile's (mean, M2) per column; the two final layers add their bias and store rcnn_cls / rcnn_reg.
// Backward, from the top, two launches per depth:
//   data      for a layer l: da_l = sum over the layers m that read a_l (the shared activation has two: cls, then reg) of dz_m . W_m, with
//             dz_m = gamma * invstd * (dy - S1 / R - xhat * S2 / R) formed in LDS from the saved z_m, dy_m and the per-tile sums S1 = sum dy,
//             S2 = sum dy * xhat merged in tile order (dz_m = the upstream gradient for a final layer); B is read straight from the
//             unpacked [cout][cin] weight.  It stores dy_l = da_l * mask * keep_scale * (y_l > 0) and the tile's S1, S2 of layer l.
//             The first layer's input gets no gradient.
//   weight    dW_m = dz_m^T . a_prev, contracted over the rows, one workgroup per 64 x 64 tile of dW; a_prev is recomputed from the saved
//             z, the statistics and the mask.  The workgroups of the first column block also store dgamma = S2, dbeta = S1, or the bias
//             gradient of a final layer.
// No atomics, no split-K through memory, no zero-fill: every output element and every word of scratch has one owner, scratch is written
// before it is read (rows past R and columns past a width are never addressed), and every sum has a fixed order: same inputs, same bits.
#include "s2d_common.h"

namespace s2d {

typedef float rt_f32x4 __attribute__((ext_vector_type(4)));

constexpr int RT_ROWS = 16;             // rows of a tile = the M of the instruction
constexpr int RT_MAXW = 256;            // widest hidden layer = channels of one staged chunk
constexpr int RT_PITCH = RT_MAXW + 4;   // LDS row pitch
constexpr int RT_MAXCIN = 4096;
constexpr int RT_MINROWS = 2, RT_MAXROWS = 8192;
constexpr int RT_WT = 64;               // a weight-gradient workgroup's tile of dW is RT_WT x RT_WT
constexpr int RT_WPITCH = RT_WT + 4;
constexpr int RT_MAXJOBS = 4;
// Sums are two-level: RT_BLOCK instructions (64 terms) accumulate in a fresh register tile that is then added to the total, so that the
// rounding error of a 2560-term product grows with the block length and the block count, not with their product.
constexpr int RT_BLOCK = 16;

// scratch of one hidden layer, in floats from the start of the workspace
struct RtOff {
    int64_t z;       // [R][cout]            pre-norm activations
    int64_t stats;   // [tiles][2][cout]     per-tile mean, M2
    int64_t col;     // [2][cout]            batch mean, invstd
    int64_t dy;      // [R][cout]            gradient at the batch norm's output
    int64_t part;    // [tiles][2][cout]     per-tile sum dy, sum dy * xhat
};

struct RtCtx {
    s2d_roi_mlp_plan plan;
    s2d_roi_mlp_train_args args;
    RtOff off[S2D_ROI_MLP_MAX_LAYERS];
    const float *feats, *packed;
    float *ws;
    const float *d_out[2];   // upstream gradients of rcnn_cls [R][1], rcnn_reg [R][7]
    float *out[2];           // rcnn_cls, rcnn_reg
    int64_t rows;
    int tiles;
};

struct RtJobs {
    int n;
    int layer[RT_MAXJOBS];
    int writer[RT_MAXJOBS];   // forward: this job's tile-0 workgroup stores (mean, invstd) and the running statistics of the layer it reads
};

__host__ __device__ inline bool rt_final(const s2d_roi_mlp_plan &p, int l) { return l == p.n_shared + p.n_cls || l == p.num_layers - 1; }
// the layer whose output layer l reads; -1: the features
__host__ __device__ inline int rt_prev(const s2d_roi_mlp_plan &p, int l) {
    return (l == p.n_shared || l == p.n_shared + p.n_cls + 1) ? p.n_shared - 1 : l - 1;
}

__device__ __forceinline__ float rt_xhat(float z, float mean, float invstd) { return (z - mean) * invstd; }
__device__ __forceinline__ float rt_y(float z, float mean, float invstd, float gamma, float beta) { return rt_xhat(z, mean, invstd) * gamma + beta; }

// Chan's merge of the per-tile (count, mean, M2) of one column, in tile order
__device__ __forceinline__ void rt_merge_stats(const float *__restrict__ stats, int tiles, int width, int64_t rows, int col, float &mean, float &m2) {
    float n = 0.f;
    mean = 0.f, m2 = 0.f;
    for (int t = 0; t < tiles; ++t) {
        const float nb = (float)min((int64_t)RT_ROWS, rows - (int64_t)t * RT_ROWS);
        const float mb = stats[((int64_t)t * 2 + 0) * width + col], vb = stats[((int64_t)t * 2 + 1) * width + col];
        const float tot = n + nb, delta = mb - mean;
        mean = mean + delta * (nb / tot);
        m2 = m2 + vb + delta * delta * (n * nb / tot);
        n = tot;
    }
}

// sum of the per-tile (S1, S2) of one column, in tile order
__device__ __forceinline__ void rt_merge_sums(const float *__restrict__ part, int tiles, int width, int col, float &s1, float &s2) {
    s1 = 0.f, s2 = 0.f;
    for (int t = 0; t < tiles; ++t) {
        s1 = s1 + part[((int64_t)t * 2 + 0) * width + col];
        s2 = s2 + part[((int64_t)t * 2 + 1) * width + col];
    }
}

// ---- forward: one layer per blockIdx.y ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rt_fwd_kernel(RtCtx c, RtJobs jobs) {
    __shared__ float a_lds[RT_ROWS * RT_PITCH];
    __shared__ float o_lds[RT_ROWS * RT_PITCH];
    __shared__ float k_mean[RT_MAXW], k_inv[RT_MAXW], k_gamma[RT_MAXW], k_beta[RT_MAXW];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l = jobs.layer[blockIdx.y];
    const s2d_roi_mlp_layer L = c.plan.layer[l];
    const int p = rt_prev(c.plan, l);
    const bool fin = rt_final(c.plan, l);
    const int64_t rows = c.rows, r0 = (int64_t)blockIdx.x * RT_ROWS;
    const int cin = L.cin;
    const float *__restrict__ in = c.feats;
    const uint8_t *__restrict__ mask = nullptr;
    float keep = 1.f;
    if (p >= 0) {   // cin <= 256: one column per thread
        const s2d_roi_mlp_train_layer P = c.args.layer[p];
        in = c.ws + c.off[p].z;
        mask = P.mask, keep = P.keep_scale;
        if (tid < cin) {
            float mean, m2;
            rt_merge_stats(c.ws + c.off[p].stats, c.tiles, cin, rows, tid, mean, m2);
            const float invstd = 1.f / sqrtf(m2 / (float)rows + P.eps);
            k_mean[tid] = mean, k_inv[tid] = invstd, k_gamma[tid] = P.gamma[tid], k_beta[tid] = P.beta[tid];
            if (jobs.writer[blockIdx.y] && blockIdx.x == 0) {
                float *col = c.ws + c.off[p].col;
                col[tid] = mean, col[cin + tid] = invstd;
                P.running_mean[tid] = (1.f - P.momentum) * P.running_mean[tid] + P.momentum * mean;
                P.running_var[tid] = (1.f - P.momentum) * P.running_var[tid] + P.momentum * (m2 / (float)(rows - 1));
            }
        }
    }
    const int tiles = L.cout_pad / 16;
    int toff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) toff[j] = 64 * min(wid + 4 * j, tiles - 1);   // a wave without a j-th tile repeats the last one and drops it
    rt_f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = rt_f32x4{0.f, 0.f, 0.f, 0.f};
    const float *__restrict__ w = c.packed + L.w_off + lane;
    const int64_t tiles64 = (int64_t)tiles * 64;
    for (int k0 = 0; k0 < cin; k0 += RT_MAXW) {
        const int cw = min(RT_MAXW, cin - k0);
        __syncthreads();   // the constants are written; the previous chunk's products have read a_lds
        for (int idx = tid; idx < RT_ROWS * cw; idx += 256) {
            const int row = idx / cw, col = idx - row * cw;
            const int64_t r = r0 + row;
            float v = 0.f;
            if (r < rows) {
                v = in[r * cin + k0 + col];
                if (p >= 0) {
                    v = rt_y(v, k_mean[col], k_inv[col], k_gamma[col], k_beta[col]);
                    v = v < 0.f ? 0.f : v;
                    if (mask) v = mask[r * cin + col] ? v * keep : 0.f;
                }
            }
            a_lds[row * RT_PITCH + col] = v;
        }
        __syncthreads();
        const float *a = a_lds + (lane & 15) * RT_PITCH + (lane >> 4);
        const int s0 = k0 / 4, steps = cw / 4;
        for (int sb = 0; sb < steps; sb += RT_BLOCK) {   // RT_BLOCK steps into a fresh accumulator, then into the total
            const int se = min(steps, sb + RT_BLOCK);
            rt_f32x4 part[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) part[j] = rt_f32x4{0.f, 0.f, 0.f, 0.f};
            // the block's weight fragments are all requested before the first product: one load latency per block, not per step
            float b[RT_BLOCK][4], av[RT_BLOCK];
#pragma unroll
            for (int u = 0; u < RT_BLOCK; ++u) {
                const bool on = sb + u < se;   // (steps past the chunk multiply zeros)
                av[u] = on ? a[4 * (sb + u)] : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) b[u][j] = on ? w[(int64_t)(s0 + sb + u) * tiles64 + toff[j]] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < RT_BLOCK; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], b[u][j], part[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = acc[j] + part[j];
        }
    }
    // C/D layout: column = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = wid + 4 * j;
        if (t < tiles) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) o_lds[(4 * (lane >> 4) + reg) * RT_PITCH + 16 * t + (lane & 15)] = acc[j][reg];
        }
    }
    __syncthreads();
    const int cout = L.cout;
    if (fin) {
        const float *__restrict__ bias = c.args.layer[l].bias;
        float *__restrict__ result = c.out[l == c.plan.num_layers - 1 ? 1 : 0];
        for (int idx = tid; idx < RT_ROWS * cout; idx += 256) {
            const int row = idx / cout, n = idx - row * cout;
            if (r0 + row < rows) result[(r0 + row) * cout + n] = o_lds[row * RT_PITCH + n] + bias[n];
        }
        return;
    }
    float *__restrict__ z = c.ws + c.off[l].z;
    for (int idx = tid; idx < RT_ROWS * cout; idx += 256) {
        const int row = idx / cout, n = idx - row * cout;
        if (r0 + row < rows) z[(r0 + row) * cout + n] = o_lds[row * RT_PITCH + n];
    }
    if (tid < cout) {   // this tile's mean and M2 of column tid over its valid rows
        const int cnt = (int)min((int64_t)RT_ROWS, rows - r0);
        float sum = 0.f;
        for (int row = 0; row < cnt; ++row) sum = sum + o_lds[row * RT_PITCH + tid];
        const float mean = sum / (float)cnt;
        float m2 = 0.f;
        for (int row = 0; row < cnt; ++row) {
            const float d = o_lds[row * RT_PITCH + tid] - mean;
            m2 = m2 + d * d;
        }
        float *stats = c.ws + c.off[l].stats;
        stats[((int64_t)blockIdx.x * 2 + 0) * cout + tid] = mean;
        stats[((int64_t)blockIdx.x * 2 + 1) * cout + tid] = m2;
    }
}

// ---- backward, data gradient: da of one hidden layer per blockIdx.y, stored as dy with the tile's sums ------------------------------------
__global__ __launch_bounds__(256) void rt_dgrad_kernel(RtCtx c, RtJobs jobs) {
    __shared__ float dz_lds[RT_ROWS * RT_PITCH];
    __shared__ float o_lds[RT_ROWS * RT_PITCH];
    __shared__ float k_s1[RT_MAXW], k_s2[RT_MAXW], k_mean[RT_MAXW], k_inv[RT_MAXW], k_ginv[RT_MAXW];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l = jobs.layer[blockIdx.y];
    const int width = c.plan.layer[l].cout;   // of a_l = the cin of every layer that reads it
    const int64_t rows = c.rows, r0 = (int64_t)blockIdx.x * RT_ROWS;
    const int tiles = width / 16;
    int noff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) noff[j] = 16 * min(wid + 4 * j, tiles - 1) + (lane & 15);
    rt_f32x4 total[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) total[j] = rt_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int m = l + 1; m < c.plan.num_layers; ++m) {   // the readers of a_l in layer order: cls before reg
        if (rt_prev(c.plan, m) != l) continue;
        const s2d_roi_mlp_layer M = c.plan.layer[m];
        const s2d_roi_mlp_train_layer A = c.args.layer[m];
        const bool fin = rt_final(c.plan, m);
        const int kdim = M.cout_pad;
        __syncthreads();   // the previous reader's products have read dz_lds and the constants
        if (!fin && tid < kdim) {
            float s1, s2;
            rt_merge_sums(c.ws + c.off[m].part, c.tiles, kdim, tid, s1, s2);
            const float *col = c.ws + c.off[m].col;
            k_s1[tid] = s1 / (float)rows, k_s2[tid] = s2 / (float)rows;
            k_mean[tid] = col[tid], k_inv[tid] = col[kdim + tid], k_ginv[tid] = A.gamma[tid] * col[kdim + tid];
        }
        __syncthreads();
        const float *__restrict__ dout = c.d_out[m == c.plan.num_layers - 1 ? 1 : 0];
        const float *__restrict__ zm = c.ws + c.off[m].z, *__restrict__ dym = c.ws + c.off[m].dy;
        for (int idx = tid; idx < RT_ROWS * kdim; idx += 256) {
            const int row = idx / kdim, k = idx - row * kdim;
            const int64_t r = r0 + row;
            float v = 0.f;
            if (r < rows) {
                if (fin) {
                    if (k < M.cout) v = dout[r * M.cout + k];
                } else {
                    const float xh = rt_xhat(zm[r * kdim + k], k_mean[k], k_inv[k]);
                    v = k_ginv[k] * (dym[r * kdim + k] - k_s1[k] - xh * k_s2[k]);
                }
            }
            dz_lds[row * RT_PITCH + k] = v;
        }
        __syncthreads();
        rt_f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = rt_f32x4{0.f, 0.f, 0.f, 0.f};
        const float *__restrict__ W = A.weight;   // [cout][width]
        const float *a = dz_lds + (lane & 15) * RT_PITCH + (lane >> 4);
        for (int kb = 0; kb < kdim / 4; kb += RT_BLOCK) {
            rt_f32x4 part[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) part[j] = rt_f32x4{0.f, 0.f, 0.f, 0.f};
            float b[RT_BLOCK][4], av[RT_BLOCK];   // as in the forward: the block's loads first (kdim is a multiple of 16: steps of 4)
#pragma unroll
            for (int u = 0; u < RT_BLOCK; ++u) {
                const int ks = kb + u, kr = 4 * ks + (lane >> 4);
                const bool on = ks < kdim / 4;
                av[u] = on ? a[4 * ks] : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) b[u][j] = on && kr < M.cout ? W[(int64_t)kr * width + noff[j]] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < RT_BLOCK; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], b[u][j], part[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = acc[j] + part[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) total[j] = total[j] + acc[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = wid + 4 * j;
        if (t < tiles) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) o_lds[(4 * (lane >> 4) + reg) * RT_PITCH + 16 * t + (lane & 15)] = total[j][reg];
        }
    }
    __syncthreads();   // (every wave is past its last product: dz_lds is free)
    const s2d_roi_mlp_train_layer A = c.args.layer[l];
    const float *col = c.ws + c.off[l].col;
    const float *__restrict__ zl = c.ws + c.off[l].z;
    float *__restrict__ dyl = c.ws + c.off[l].dy;
    for (int idx = tid; idx < RT_ROWS * width; idx += 256) {
        const int row = idx / width, n = idx - row * width;
        const int64_t r = r0 + row;
        float dy = 0.f, xh = 0.f;
        if (r < rows) {
            const float mean = col[n], inv = col[width + n];
            const float zv = zl[r * width + n];
            xh = rt_xhat(zv, mean, inv);
            const float y = rt_y(zv, mean, inv, A.gamma[n], A.beta[n]);
            dy = y > 0.f ? o_lds[row * RT_PITCH + n] : 0.f;
            if (A.mask) dy = A.mask[r * width + n] ? dy * A.keep_scale : 0.f;
            dyl[r * width + n] = dy;
        }
        o_lds[row * RT_PITCH + n] = dy;
        dz_lds[row * RT_PITCH + n] = xh;
    }
    __syncthreads();
    if (tid < width) {
        float s1 = 0.f, s2 = 0.f;
        for (int row = 0; row < RT_ROWS; ++row) {
            const float dy = o_lds[row * RT_PITCH + tid];
            s1 = s1 + dy;
            s2 = s2 + dy * dz_lds[row * RT_PITCH + tid];
        }
        float *part = c.ws + c.off[l].part;
        part[((int64_t)blockIdx.x * 2 + 0) * width + tid] = s1;
        part[((int64_t)blockIdx.x * 2 + 1) * width + tid] = s2;
    }
}

// ---- backward, weight gradient: one 64 x 64 tile of dW of the layer blockIdx.z per workgroup, contracted over all rows --------------------
__global__ __launch_bounds__(256) void rt_wgrad_kernel(RtCtx c, RtJobs jobs) {
    __shared__ float dz_lds[RT_ROWS * RT_WPITCH];
    __shared__ float a_lds[RT_ROWS * RT_WPITCH];
    __shared__ float k_s1[RT_WT], k_s2[RT_WT], k_mean[RT_WT], k_inv[RT_WT], k_ginv[RT_WT];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int m = jobs.layer[blockIdx.z];
    const s2d_roi_mlp_layer M = c.plan.layer[m];
    const int co0 = RT_WT * blockIdx.y, ci0 = RT_WT * blockIdx.x;
    if (ci0 >= M.cin || co0 >= M.cout_pad) return;   // (the grid is the largest job's)
    const s2d_roi_mlp_train_layer A = c.args.layer[m];
    const bool fin = rt_final(c.plan, m);
    const int p = rt_prev(c.plan, m);
    const int64_t rows = c.rows;
    const int kdim = M.cout_pad;
    if (!fin && tid < RT_WT && co0 + tid < M.cout) {
        const int co = co0 + tid;
        float s1, s2;
        rt_merge_sums(c.ws + c.off[m].part, c.tiles, kdim, co, s1, s2);
        if (blockIdx.x == 0) A.d_gamma[co] = s2, A.d_beta[co] = s1;
        const float *col = c.ws + c.off[m].col;
        k_s1[tid] = s1 / (float)rows, k_s2[tid] = s2 / (float)rows;
        k_mean[tid] = col[co], k_inv[tid] = col[kdim + co], k_ginv[tid] = A.gamma[co] * col[kdim + co];
    }
    __syncthreads();
    // element idx = tid + 256 i of a 16 x 64 tile: row tid / 64 + 4 i, column tid % 64 - a thread keeps its column
    const int colq = tid & 63, rowq = tid >> 6;
    const int co = co0 + colq, ci = ci0 + colq;
    const bool co_ok = co < M.cout, ci_ok = ci < M.cin;
    const float *__restrict__ dout = c.d_out[m == c.plan.num_layers - 1 ? 1 : 0];
    const float *__restrict__ zm = c.ws + (fin ? 0 : c.off[m].z), *__restrict__ dym = c.ws + (fin ? 0 : c.off[m].dy);
    const float *__restrict__ in = c.feats;
    const uint8_t *__restrict__ mask = nullptr;
    float keep = 1.f, pmean = 0.f, pinv = 0.f, pgamma = 0.f, pbeta = 0.f;
    if (p >= 0) {
        const s2d_roi_mlp_train_layer P = c.args.layer[p];
        in = c.ws + c.off[p].z;
        mask = P.mask, keep = P.keep_scale;
        if (ci_ok) {
            const float *pcol = c.ws + c.off[p].col;
            pmean = pcol[ci], pinv = pcol[M.cin + ci], pgamma = P.gamma[ci], pbeta = P.beta[ci];
        }
    }
    const bool wave_on = co0 + 16 * wid < M.cout_pad;
    rt_f32x4 acc[4], part[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = part[j] = rt_f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int t = 0; t < c.tiles; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = rowq + 4 * i;
            const int64_t r = (int64_t)t * RT_ROWS + row;
            float dz = 0.f, av = 0.f;
            if (r < rows && co_ok) {
                if (fin)
                    dz = dout[r * M.cout + co];
                else
                    dz = k_ginv[colq] * (dym[r * kdim + co] - k_s1[colq] - rt_xhat(zm[r * kdim + co], k_mean[colq], k_inv[colq]) * k_s2[colq]);
            }
            if (r < rows && ci_ok) {
                av = in[r * M.cin + ci];
                if (p >= 0) {
                    av = rt_y(av, pmean, pinv, pgamma, pbeta);
                    av = av < 0.f ? 0.f : av;
                    if (mask) av = mask[r * M.cin + ci] ? av * keep : 0.f;
                }
            }
            dz_lds[row * RT_WPITCH + colq] = dz;
            a_lds[row * RT_WPITCH + colq] = av;
        }
        __syncthreads();
        if (fin && blockIdx.x == 0 && tid < RT_WT)
            for (int row = 0; row < RT_ROWS; ++row) bsum = bsum + dz_lds[row * RT_WPITCH + tid];
        if (wave_on) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int kr = 4 * ks + (lane >> 4);
                const float a = dz_lds[kr * RT_WPITCH + 16 * wid + (lane & 15)];
#pragma unroll
                for (int j = 0; j < 4; ++j) part[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, a_lds[kr * RT_WPITCH + 16 * j + (lane & 15)], part[j], 0, 0, 0);
            }
            if ((t & 3) == 3 || t == c.tiles - 1) {   // four tiles = RT_BLOCK instructions = 64 rows
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = acc[j] + part[j], part[j] = rt_f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        __syncthreads();
    }
    if (wave_on) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int o = co0 + 16 * wid + 4 * (lane >> 4) + reg, i = ci0 + 16 * j + (lane & 15);
                if (o < M.cout && i < M.cin) A.d_weight[(int64_t)o * M.cin + i] = acc[j][reg];
            }
    }
    if (fin && blockIdx.x == 0 && tid < RT_WT && co_ok) A.d_bias[co] = bsum;
}

// ---- the two RoI losses (roi_head_template.py:94-151: BinaryCrossEntropy on sigmoid(x) with torch's clamp of the logarithms at -100; L1
// times code_weights over the foreground rows).  One workgroup; per-row terms in fp32 as torch forms them, sums in double in a fixed order.
struct RtLossArgs {
    const float *cls, *reg, *labels, *fg, *target;   // [R], [R][7], [R] (< 0: ignored), [R] (> 0: foreground), [R][7]
    int64_t rows;
    float code_weights[7];
    float w_cls, w_reg;
};

__device__ __forceinline__ float rt_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(256) void rt_loss_fwd_kernel(RtLossArgs a, float *__restrict__ out) {
    __shared__ double red[4][256];
    const int tid = threadIdx.x;
    double s_cls = 0., s_valid = 0., s_reg = 0., s_fg = 0.;
    for (int64_t r = tid; r < a.rows; r += 256) {
        const float y = a.labels[r];
        if (y >= 0.f) {
            const float pr = rt_sigmoid(a.cls[r]);
            const float lp = fmaxf(logf(pr), -100.f), lq = fmaxf(logf(1.f - pr), -100.f);
            s_cls += (double)(-(y * lp + (1.f - y) * lq));
            s_valid += 1.;
        }
        if (a.fg[r] > 0.f) {
            float row = 0.f;
#pragma unroll
            for (int k = 0; k < 7; ++k) row = row + fabsf(a.reg[r * 7 + k] - a.target[r * 7 + k]) * a.code_weights[k];
            s_reg += (double)row;
            s_fg += 1.;
        }
    }
    red[0][tid] = s_cls, red[1][tid] = s_valid, red[2][tid] = s_reg, red[3][tid] = s_fg;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + half];
        __syncthreads();
    }
    if (tid == 0) {
        const double valid = red[1][0] < 1. ? 1. : red[1][0], fg = red[3][0] < 1. ? 1. : red[3][0];
        out[0] = (float)(red[0][0] / valid * (double)a.w_cls);
        out[1] = (float)(red[2][0] / fg * (double)a.w_reg);
        out[2] = (float)red[1][0];
        out[3] = (float)red[3][0];
    }
}

// torch's backward of the same: BCE (p - y) / max(p (1 - p), 1e-12), sigmoid p (1 - p); L1 sign(reg - target)
__global__ __launch_bounds__(256) void rt_loss_bwd_kernel(RtLossArgs a, const float *__restrict__ out, const float *__restrict__ g_cls,
                                                          const float *__restrict__ g_reg, float *__restrict__ d_cls, float *__restrict__ d_reg) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.rows) return;
    const float gc = g_cls[0] * a.w_cls / fmaxf(out[2], 1.f), gr = g_reg[0] * a.w_reg / fmaxf(out[3], 1.f);
    const float y = a.labels[r];
    float d = 0.f;
    if (y >= 0.f) {
        const float pr = rt_sigmoid(a.cls[r]);
        const float v = pr * (1.f - pr);
        d = gc * (pr - y) / fmaxf(v, 1e-12f) * v;
    }
    d_cls[r] = d;
    const bool fg = a.fg[r] > 0.f;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const float diff = a.reg[r * 7 + k] - a.target[r * 7 + k];
        const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
        d_reg[r * 7 + k] = fg ? gr * a.code_weights[k] * sgn : 0.f;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
static bool rt_plan_ok(const s2d_roi_mlp_plan *p) {   // the checks of roi_mlp.hip's table that the kernels above rely on
    if (!p || p->n_shared < 1 || p->n_shared > 2 || p->n_cls < 0 || p->n_cls > 2 || p->n_reg < 0 || p->n_reg > 2) return false;
    if (p->num_layers != p->n_shared + p->n_cls + p->n_reg + 2) return false;
    int64_t w = 0;
    for (int l = 0; l < p->num_layers; ++l) {
        const s2d_roi_mlp_layer &L = p->layer[l];
        const bool fin = rt_final(*p, l);
        if (L.cin < 4 || L.cin % 4 != 0 || L.cin > (l == 0 ? RT_MAXCIN : RT_MAXW) || (l > 0 && L.cin % 16 != 0)) return false;
        if (fin ? (L.cout_pad != 16 || L.cout != (l == p->num_layers - 1 ? 7 : 1) || L.relu)
                : (L.cout < 16 || L.cout > RT_MAXW || L.cout % 16 != 0 || L.cout_pad != L.cout || !L.relu)) return false;
        if (L.w_off != w) return false;
        w += (int64_t)L.cin * L.cout_pad;
        if (l > 0 && L.cin != p->layer[rt_prev(*p, l)].cout) return false;
    }
    return w == p->packed_elems;
}

static bool rt_rows_ok(int64_t rows) { return rows >= RT_MINROWS && rows <= RT_MAXROWS; }

// fills off[] for the hidden layers; returns the workspace size in floats
static int64_t rt_layout(const s2d_roi_mlp_plan &p, int64_t rows, RtOff *off) {
    const int64_t tiles = ceil_div(rows, RT_ROWS);
    int64_t at = 0;
    for (int l = 0; l < p.num_layers; ++l) {
        RtOff o = {0, 0, 0, 0, 0};
        if (!rt_final(p, l)) {
            const int64_t w = p.layer[l].cout;
            o.z = at, at += rows * w;
            o.stats = at, at += tiles * 2 * w;
            o.col = at, at += 2 * w;
            o.dy = at, at += rows * w;
            o.part = at, at += tiles * 2 * w;
        }
        if (off) off[l] = o;
    }
    return at;
}

static int rt_ctx(RtCtx &c, const s2d_roi_mlp_plan *plan, const s2d_roi_mlp_train_args *args, const float *feats, int64_t rows, void *ws,
                  size_t ws_bytes, bool backward) {
    S2D_CHECK_ARG(rt_plan_ok(plan), "roi_mlp_train: not a plan of s2d_roi_mlp_plan_make");
    S2D_CHECK_ARG(rt_rows_ok(rows), "roi_mlp_train: %lld rows (%d .. %d)", (long long)rows, RT_MINROWS, RT_MAXROWS);
    S2D_CHECK_ARG(args && feats && ws, "roi_mlp_train: null argument");
    memset(&c, 0, sizeof(c));
    c.plan = *plan, c.args = *args, c.feats = feats, c.ws = (float *)ws, c.rows = rows, c.tiles = (int)ceil_div(rows, RT_ROWS);
    S2D_CHECK_ARG(ws_bytes >= (size_t)rt_layout(*plan, rows, c.off) * sizeof(float), "roi_mlp_train: workspace of %zu bytes is too small", ws_bytes);
    for (int l = 0; l < plan->num_layers; ++l) {
        const s2d_roi_mlp_train_layer &A = args->layer[l];
        S2D_CHECK_ARG(A.weight, "roi_mlp_train: null weight of layer %d", l);
        if (rt_final(*plan, l)) {
            S2D_CHECK_ARG(A.bias && (!backward || (A.d_weight && A.d_bias)), "roi_mlp_train: null bias or gradient of final layer %d", l);
        } else {
            S2D_CHECK_ARG(A.gamma && A.beta && A.running_mean && A.running_var, "roi_mlp_train: null batch norm tensor of layer %d", l);
            S2D_CHECK_ARG(!backward || (A.d_weight && A.d_gamma && A.d_beta), "roi_mlp_train: null gradient of layer %d", l);
            S2D_CHECK_ARG(A.keep_scale >= 1.f && A.keep_scale < 3.4e38f && A.eps > 0.f && A.momentum >= 0.f && A.momentum <= 1.f,
                          "roi_mlp_train: keep_scale %g, eps %g, momentum %g of layer %d", A.keep_scale, A.eps, A.momentum, l);
        }
    }
    return S2D_OK;
}

}  // namespace s2d

using namespace s2d;

extern "C" int s2d_roi_mlp_train_supported(int cin, int n_shared, int s0, int s1, int n_cls, int c0, int c1, int n_reg, int r0, int r1, int num_class,
                                           int code_size, int64_t rows, float dp_ratio) {
    if (!s2d_roi_mlp_supported(cin, n_shared, s0, s1, n_cls, c0, c1, n_reg, r0, r1, num_class, code_size)) return 0;
    return rt_rows_ok(rows) && dp_ratio < 1.f ? 1 : 0;   // (a negative ratio builds no dropout site; NaN is refused)
}

extern "C" size_t s2d_roi_mlp_train_scratch_bytes(const s2d_roi_mlp_plan *plan, int64_t rows) {
    if (!rt_plan_ok(plan) || !rt_rows_ok(rows)) return 0;
    return (size_t)rt_layout(*plan, rows, nullptr) * sizeof(float);
}

extern "C" int s2d_roi_mlp_train_launches(const s2d_roi_mlp_plan *plan, int *forward, int *backward) {
    S2D_CHECK_ARG(rt_plan_ok(plan) && forward && backward, "roi_mlp_train_launches: bad argument");
    const int branch = plan->n_cls > plan->n_reg ? plan->n_cls : plan->n_reg;
    *forward = plan->n_shared + branch + 1;
    *backward = 2 * (plan->n_shared + branch);   // a data and a weight launch per level
    return S2D_OK;
}

extern "C" int s2d_roi_mlp_train_forward(const s2d_roi_mlp_plan *plan, const s2d_roi_mlp_train_args *args, const float *feats, int64_t rows,
                                         const float *packed, void *workspace, size_t workspace_bytes, float *rcnn_cls, float *rcnn_reg,
                                         s2d_stream_t stream) {
    RtCtx local;
    int rc = rt_ctx(local, plan, args, feats, rows, workspace, workspace_bytes, false);
    if (rc != S2D_OK) return rc;
    S2D_CHECK_ARG(packed && rcnn_cls && rcnn_reg, "roi_mlp_train_forward: null argument");
    local.packed = packed, local.out[0] = rcnn_cls, local.out[1] = rcnn_reg;
    bool written[S2D_ROI_MLP_MAX_LAYERS] = {false};
    auto launch = [&](RtJobs &jobs) {
        for (int j = 0; j < jobs.n; ++j) {
            const int p = rt_prev(*plan, jobs.layer[j]);
            jobs.writer[j] = p >= 0 && !written[p];
            if (p >= 0) written[p] = true;
        }
        hipLaunchKernelGGL(rt_fwd_kernel, dim3((unsigned)local.tiles, (unsigned)jobs.n), dim3(256), 0, (hipStream_t)stream, local, jobs);
    };
    for (int d = 0; d < plan->n_shared; ++d) {
        RtJobs jobs = {1, {d, 0, 0, 0}, {0, 0, 0, 0}};
        launch(jobs);
        S2D_LAUNCH_CHECK();
    }
    const int cls0 = plan->n_shared, reg0 = plan->n_shared + plan->n_cls + 1;
    for (int h = 0; h < 2; ++h) {
        RtJobs jobs = {0, {0, 0, 0, 0}, {0, 0, 0, 0}};
        if (h < plan->n_cls) jobs.layer[jobs.n++] = cls0 + h;
        if (h < plan->n_reg) jobs.layer[jobs.n++] = reg0 + h;
        if (jobs.n == 0) break;
        launch(jobs);
        S2D_LAUNCH_CHECK();
    }
    RtJobs jobs = {2, {cls0 + plan->n_cls, plan->num_layers - 1, 0, 0}, {0, 0, 0, 0}};
    launch(jobs);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_roi_mlp_train_backward(const s2d_roi_mlp_plan *plan, const s2d_roi_mlp_train_args *args, const float *feats, int64_t rows,
                                          void *workspace, size_t workspace_bytes, const float *d_rcnn_cls, const float *d_rcnn_reg,
                                          s2d_stream_t stream) {
    RtCtx c;
    int rc = rt_ctx(c, plan, args, feats, rows, workspace, workspace_bytes, true);
    if (rc != S2D_OK) return rc;
    S2D_CHECK_ARG(d_rcnn_cls && d_rcnn_reg, "roi_mlp_train_backward: null argument");
    c.d_out[0] = d_rcnn_cls, c.d_out[1] = d_rcnn_reg;
    // level of a hidden layer: 1 + the highest level among the hidden layers that read it (readers have higher indices)
    int level[S2D_ROI_MLP_MAX_LAYERS] = {0}, top = 0;
    for (int l = plan->num_layers - 1; l >= 0; --l) {
        if (rt_final(*plan, l)) continue;
        int lv = 1;
        for (int m = l + 1; m < plan->num_layers; ++m)
            if (rt_prev(*plan, m) == l && !rt_final(*plan, m) && level[m] + 1 > lv) lv = level[m] + 1;
        level[l] = lv;
        if (lv > top) top = lv;
    }
    for (int k = 1; k <= top; ++k) {
        RtJobs dj = {0, {0, 0, 0, 0}, {0, 0, 0, 0}}, wj = {0, {0, 0, 0, 0}, {0, 0, 0, 0}};
        for (int l = 0; l < plan->num_layers; ++l) {
            if (rt_final(*plan, l) ? k == 1 : level[l] == k) wj.layer[wj.n++] = l;
            if (!rt_final(*plan, l) && level[l] == k) dj.layer[dj.n++] = l;
        }
        hipLaunchKernelGGL(rt_dgrad_kernel, dim3((unsigned)c.tiles, (unsigned)dj.n), dim3(256), 0, (hipStream_t)stream, c, dj);
        S2D_LAUNCH_CHECK();
        int gx = 1, gy = 1;
        for (int j = 0; j < wj.n; ++j) {
            const s2d_roi_mlp_layer &L = plan->layer[wj.layer[j]];
            gx = (int)ceil_div(L.cin, RT_WT) > gx ? (int)ceil_div(L.cin, RT_WT) : gx;
            gy = (int)ceil_div(L.cout_pad, RT_WT) > gy ? (int)ceil_div(L.cout_pad, RT_WT) : gy;
        }
        hipLaunchKernelGGL(rt_wgrad_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)wj.n), dim3(256), 0, (hipStream_t)stream, c, wj);
        S2D_LAUNCH_CHECK();
    }
    return S2D_OK;
}

static int rt_loss_args(RtLossArgs &a, const float *cls, const float *reg, const float *labels, const float *fg, const float *target, int64_t rows,
                        const float *code_weights, float w_cls, float w_reg) {
    S2D_CHECK_ARG(rows >= 1 && rows < (1ll << 31) && cls && reg && labels && fg && target && code_weights, "roi_loss: %lld rows or a null argument",
                  (long long)rows);
    a.cls = cls, a.reg = reg, a.labels = labels, a.fg = fg, a.target = target, a.rows = rows, a.w_cls = w_cls, a.w_reg = w_reg;
    for (int k = 0; k < 7; ++k) a.code_weights[k] = code_weights[k];
    return S2D_OK;
}

extern "C" int s2d_roi_loss_forward(const float *rcnn_cls, const float *rcnn_reg, const float *labels, const float *fg, const float *target,
                                    int64_t rows, const float *code_weights, float w_cls, float w_reg, float *out, s2d_stream_t stream) {
    RtLossArgs a;
    int rc = rt_loss_args(a, rcnn_cls, rcnn_reg, labels, fg, target, rows, code_weights, w_cls, w_reg);
    if (rc != S2D_OK) return rc;
    S2D_CHECK_ARG(out, "roi_loss_forward: null out");
    hipLaunchKernelGGL(rt_loss_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, out);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_roi_loss_backward(const float *rcnn_cls, const float *rcnn_reg, const float *labels, const float *fg, const float *target,
                                     int64_t rows, const float *code_weights, float w_cls, float w_reg, const float *out, const float *g_cls,
                                     const float *g_reg, float *d_rcnn_cls, float *d_rcnn_reg, s2d_stream_t stream) {
    RtLossArgs a;
    int rc = rt_loss_args(a, rcnn_cls, rcnn_reg, labels, fg, target, rows, code_weights, w_cls, w_reg);
    if (rc != S2D_OK) return rc;
    S2D_CHECK_ARG(out && g_cls && g_reg && d_rcnn_cls && d_rcnn_reg, "roi_loss_backward: null argument");
    hipLaunchKernelGGL(rt_loss_bwd_kernel, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, (hipStream_t)stream, a, out, g_cls, g_reg, d_rcnn_cls,
                       d_rcnn_reg);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
