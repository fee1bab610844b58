// The eval-mode RoI MLP of the two-stage head in ONE launch, exact fp32 on the matrix cores:
//   feats [R][cin] -> shared_fc_layer (1-2 x Conv1d(k=1) + BatchNorm1d + ReLU) -> cls_layers / reg_layers (0-2 such layers each, then a
//   Conv1d with bias) -> rcnn_cls [R][1], rcnn_reg [R][7]
// (det3d/models/roi_heads/roi_head.py:16-106 of the reference, roi_head_template.py:27-41 make_fc_layers; the torch chain ran it as eight
// convolutions, six batch norms and six ReLUs over a [R][C][1] tensor, ~28 launches).  Every layer is y = act(scale[c] * (x . W^T)[c] +
// shift[c]); scale and shift are applied in the epilogue (one multiply, one add, -ffp-contract=off), never folded into the weights, so the
// products round as the chain's convolution rounds them and a changed running statistic needs no re-pack.
//
// A workgroup of 4 waves owns 16 rows.  One v_mfma_f32_16x16x4_f32 contracts 4 input channels for a 16-row x 16-column tile: lane l
// supplies A = x[row l & 15][k0 + (l >> 4)] (one LDS dword) and B = W[n0 + (l & 15)][k0 + (l >> 4)] (one global dword: the packed image
// stores, per 4-channel step and 16-column tile, the 64 lanes' values in lane order, so a wave's load is 256 contiguous bytes and the
// workgroup's loads of one step are one contiguous run).  Wave w owns column tiles w, w + 4, w + 8, w + 12: at width 256 four independent
// accumulators (the instruction's dependent latency is 40 cycles against a 32-cycle issue interval).  The weight fragments of the next 8
// steps are in flight while the current 8 are multiplied.
// First layer: the row tile's features are staged through LDS in chunks of 128 channels, double-buffered (the next chunk's global loads
// are issued before the current chunk's products and written behind them); a cin that is no multiple of the chunk or of 8 steps ends in
// single steps; columns past cin and rows past R are loaded as zeros.  Later layers: the [16][<= 256] activations stay in LDS (three
// buffers: the shared activation is kept while a branch ping-pongs between the other two; the first layer's staging aliases those two).
// The two final convolutions (1 and 7 columns) are one zero-padded 16-column tile each.
// No split-K, no atomics, no zero-fill: every output element has one owner; a row's result depends on that row only and on nothing else
// in the call (the order of its sum is fixed by cin alone).
#include "s2d_common.h"

namespace s2d {

typedef float rm_f32x4 __attribute__((ext_vector_type(4)));

constexpr int RM_ROWS = 16;                 // rows of a workgroup's tile = the M of the instruction
constexpr int RM_MAXW = 256;                // widest hidden layer
constexpr int RM_PITCH = RM_MAXW + 4;       // LDS row pitch of an activation buffer: 16 rows x 4 k-lanes fall on 64 different banks
constexpr int RM_CHUNK = 128;               // input channels of one staged chunk of the first layer
constexpr int RM_SPITCH = RM_CHUNK + 4;     // its row pitch (a multiple of 4 floats: 16-byte LDS stores)
constexpr int RM_U = 8;                     // 4-channel steps whose weight fragments are fetched together
constexpr int RM_MAXCIN = 4096;

struct RmPackSrc {
    const float *w[S2D_ROI_MLP_MAX_LAYERS];
};

// packed[w_off + (ks * tiles + t) * 64 + l] = W[16 t + (l & 15)][4 ks + (l >> 4)], zero for the rows past cout (the final layers' padding)
__global__ __launch_bounds__(256) void roi_mlp_pack_kernel(s2d_roi_mlp_plan plan, RmPackSrc src, float *__restrict__ packed) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= plan.packed_elems) return;
    int l = 0;
    while (l + 1 < plan.num_layers && e >= plan.layer[l + 1].w_off) ++l;
    const s2d_roi_mlp_layer L = plan.layer[l];
    const int64_t local = e - L.w_off;
    const int lane = (int)(local & 63), tiles = L.cout_pad / 16;
    const int64_t frag = local >> 6;
    const int t = (int)(frag % tiles);
    const int64_t ks = frag / tiles;
    const int n = 16 * t + (lane & 15);
    const int64_t k = 4 * ks + (lane >> 4);
    packed[e] = n < L.cout ? src.w[l][(int64_t)n * L.cin + k] : 0.f;
}

template <int J>
__device__ __forceinline__ void rm_fetch(float (&b)[RM_U][J], const float *__restrict__ w, int64_t step, int tiles64, const int (&toff)[J]) {
#pragma unroll
    for (int u = 0; u < RM_U; ++u)
#pragma unroll
        for (int j = 0; j < J; ++j) b[u][j] = w[(step + u) * tiles64 + toff[j]];
}

template <int J, int N>
__device__ __forceinline__ void rm_multiply(rm_f32x4 (&acc)[4], const float *a, const float (&b)[RM_U][J]) {
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const float av = a[4 * u];
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[u][j], acc[j], 0, 0, 0);
    }
}

// a layer whose input lies in LDS: a = &in[(lane & 15) * RM_PITCH + (lane >> 4)], w = image of the layer + lane, steps = cin / 4 (a
// multiple of 4: hidden widths are multiples of 16)
template <int J>
__device__ __forceinline__ void rm_gemm_lds(rm_f32x4 (&acc)[4], const float *a, const float *__restrict__ w, int steps, int tiles64, const int (&toff)[J]) {
    const int groups = steps / RM_U;
    float bn[RM_U][J];
    if (groups > 0) rm_fetch<J>(bn, w, 0, tiles64, toff);
    for (int g = 0; g < groups; ++g) {
        float bc[RM_U][J];
#pragma unroll
        for (int u = 0; u < RM_U; ++u)
#pragma unroll
            for (int j = 0; j < J; ++j) bc[u][j] = bn[u][j];
        if (g + 1 < groups) rm_fetch<J>(bn, w, (int64_t)(g + 1) * RM_U, tiles64, toff);
        rm_multiply<J, RM_U>(acc, a + 4 * RM_U * g, bc);
    }
    for (int s = groups * RM_U; s < steps; ++s) {
        const float av = a[4 * s];
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[(int64_t)s * tiles64 + toff[j]], acc[j], 0, 0, 0);
    }
}

// the first layer: feats rows r0 .. r0 + 15 through the two staging buffers
template <int J>
__device__ __forceinline__ void rm_gemm_first(rm_f32x4 (&acc)[4], const float *__restrict__ feats, int64_t r0, int64_t rows, int cin, float *stage0,
                                              float *stage1, const float *__restrict__ w, int tiles64, const int (&toff)[J]) {
    const int lane = threadIdx.x & 63;
    const int steps = cin / 4, groups = steps / RM_U, chunks = (cin + RM_CHUNK - 1) / RM_CHUNK;
    // thread -> two 16-byte pieces of the chunk: piece p = threadIdx.x + 256 i -> row p / 32, channels 4 (p % 32) ..
    const int prow[2] = {(int)threadIdx.x / 32, (int)threadIdx.x / 32 + 8};
    const int pcol = 4 * ((int)threadIdx.x % 32);
    auto load_chunk = [&](int c, rm_f32x4 (&v)[2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t r = r0 + prow[i];
            const int col = c * RM_CHUNK + pcol;
            v[i] = (r < rows && col < cin) ? *reinterpret_cast<const rm_f32x4 *>(feats + r * cin + col) : rm_f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_chunk = [&](float *stage, const rm_f32x4 (&v)[2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<rm_f32x4 *>(stage + prow[i] * RM_SPITCH + pcol) = v[i];
    };
    rm_f32x4 v[2];
    load_chunk(0, v);
    store_chunk(stage0, v);
    float bn[RM_U][J];
    if (groups > 0) rm_fetch<J>(bn, w, 0, tiles64, toff);
    __syncthreads();
    const int aoff = (lane & 15) * RM_SPITCH + (lane >> 4);
    for (int c = 0; c < chunks; ++c) {
        const float *a = ((c & 1) ? stage1 : stage0) + aoff;
        if (c + 1 < chunks) load_chunk(c + 1, v);
        const int s0 = c * (RM_CHUNK / 4);
        const int s1 = min(steps, s0 + RM_CHUNK / 4);
        const int g1 = min(groups, (c + 1) * (RM_CHUNK / 4 / RM_U));
        for (int g = c * (RM_CHUNK / 4 / RM_U); g < g1; ++g) {
            float bc[RM_U][J];
#pragma unroll
            for (int u = 0; u < RM_U; ++u)
#pragma unroll
                for (int j = 0; j < J; ++j) bc[u][j] = bn[u][j];
            if (g + 1 < groups) rm_fetch<J>(bn, w, (int64_t)(g + 1) * RM_U, tiles64, toff);
            rm_multiply<J, RM_U>(acc, a + 4 * (g * RM_U - s0), bc);
        }
        for (int s = max(s0, groups * RM_U); s < s1; ++s) {   // the steps behind the last whole group (they lie in the last chunk)
            const float av = a[4 * (s - s0)];
#pragma unroll
            for (int j = 0; j < J; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[(int64_t)s * tiles64 + toff[j]], acc[j], 0, 0, 0);
        }
        if (c + 1 < chunks) store_chunk((c & 1) ? stage0 : stage1, v);
        __syncthreads();
    }
}

// one layer for this wave's column tiles: product, then scale / shift / ReLU into `out` (hidden layers) or to global memory (final layers)
template <int J>
__device__ __forceinline__ void rm_layer(const s2d_roi_mlp_layer &L, bool first, const float *__restrict__ feats, int64_t r0, int64_t rows, float *stage0,
                                         float *stage1, const float *in, float *out, const float *__restrict__ packed,
                                         const float *__restrict__ affine, float *__restrict__ result, int result_cols) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int tiles = L.cout_pad / 16;
    int toff[J];
#pragma unroll
    for (int j = 0; j < J; ++j) toff[j] = 64 * min(wid + 4 * j, tiles - 1);   // a wave without a j-th tile repeats the last one and drops it
    rm_f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = rm_f32x4{0.f, 0.f, 0.f, 0.f};
    const float *w = packed + L.w_off + lane;
    if (first)
        rm_gemm_first<J>(acc, feats, r0, rows, L.cin, stage0, stage1, w, tiles * 64, toff);
    else
        rm_gemm_lds<J>(acc, in + (lane & 15) * RM_PITCH + (lane >> 4), w, L.cin / 4, tiles * 64, toff);
    // C/D layout: column = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int t = wid + 4 * j;
        if (t >= tiles) continue;
        const int n = 16 * t + (lane & 15);
        const float sc = affine[L.affine_off + n], sh = affine[L.affine_off + L.cout_pad + n];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = 4 * (lane >> 4) + reg;
            float y = acc[j][reg] * sc;
            y = y + sh;
            if (L.relu) y = y < 0.f ? 0.f : y;   // (keeps a NaN, as torch's ReLU does)
            if (result == nullptr)
                out[row * RM_PITCH + n] = y;
            else if (n < result_cols && r0 + row < rows)
                result[(r0 + row) * result_cols + n] = y;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void rm_layer_any(const s2d_roi_mlp_layer &L, bool first, const float *__restrict__ feats, int64_t r0, int64_t rows, float *stage0,
                                             float *stage1, const float *in, float *out, const float *__restrict__ packed,
                                             const float *__restrict__ affine, float *__restrict__ result, int result_cols) {
    const int per_wave = (L.cout_pad / 16 + 3) / 4;   // column tiles of the busiest wave
    if (per_wave == 1) rm_layer<1>(L, first, feats, r0, rows, stage0, stage1, in, out, packed, affine, result, result_cols);
    else if (per_wave == 2) rm_layer<2>(L, first, feats, r0, rows, stage0, stage1, in, out, packed, affine, result, result_cols);
    else if (per_wave == 3) rm_layer<3>(L, first, feats, r0, rows, stage0, stage1, in, out, packed, affine, result, result_cols);
    else rm_layer<4>(L, first, feats, r0, rows, stage0, stage1, in, out, packed, affine, result, result_cols);
}

__global__ __launch_bounds__(256) void roi_mlp_kernel(s2d_roi_mlp_plan plan, const float *__restrict__ feats, int64_t rows,
                                                      const float *__restrict__ packed, const float *__restrict__ affine,
                                                      float *__restrict__ rcnn_cls, float *__restrict__ rcnn_reg) {
    __shared__ __attribute__((aligned(16))) float act[3][RM_ROWS * RM_PITCH];
    const int64_t r0 = (int64_t)blockIdx.x * RM_ROWS;
    // shared layers: 0 -> buffer 0 (its staging lies in buffers 1 and 2), 1 -> buffer 1
    int l = 0, s = 0;
    rm_layer_any(plan.layer[0], true, feats, r0, rows, act[1], act[2], nullptr, act[0], packed, affine, nullptr, 0);
    for (l = 1; l < plan.n_shared; ++l, ++s) rm_layer_any(plan.layer[l], false, feats, r0, rows, nullptr, nullptr, act[s], act[s + 1], packed, affine, nullptr, 0);
    // the two branches read buffer s and use the other two
    for (int branch = 0; branch < 2; ++branch) {
        const int hidden = branch == 0 ? plan.n_cls : plan.n_reg;
        int in = s;
        for (int h = 0; h < hidden; ++h, ++l) {
            const int out = in == s ? (s + 1) % 3 : 3 - s - in;
            rm_layer_any(plan.layer[l], false, feats, r0, rows, nullptr, nullptr, act[in], act[out], packed, affine, nullptr, 0);
            in = out;
        }
        rm_layer_any(plan.layer[l], false, feats, r0, rows, nullptr, nullptr, act[in], nullptr, packed, affine, branch == 0 ? rcnn_cls : rcnn_reg,
                     branch == 0 ? 1 : 7);
        ++l;
    }
}

static bool rm_width_ok(int w) { return w >= 16 && w <= RM_MAXW && w % 16 == 0; }

static bool rm_supported(int cin, int n_shared, int s0, int s1, int n_cls, int c0, int c1, int n_reg, int r0, int r1, int num_class, int code_size) {
    if (cin < 4 || cin > RM_MAXCIN || cin % 4 != 0) return false;
    if (n_shared < 1 || n_shared > 2 || n_cls < 0 || n_cls > 2 || n_reg < 0 || n_reg > 2) return false;
    if (num_class != 1 || code_size != 7) return false;
    const int widths[6] = {s0, s1, c0, c1, r0, r1}, counts[3] = {n_shared, n_cls, n_reg};
    for (int g = 0; g < 3; ++g)
        for (int i = 0; i < counts[g]; ++i)
            if (!rm_width_ok(widths[2 * g + i])) return false;
    return true;
}

static bool rm_plan_ok(const s2d_roi_mlp_plan *p) {
    if (!p || p->n_shared < 1 || p->n_shared > 2 || p->n_cls < 0 || p->n_cls > 2 || p->n_reg < 0 || p->n_reg > 2) return false;
    if (p->num_layers != p->n_shared + p->n_cls + p->n_reg + 2) return false;
    int64_t w = 0;
    int a = 0;
    for (int l = 0; l < p->num_layers; ++l) {
        const s2d_roi_mlp_layer &L = p->layer[l];
        const bool fin = l == p->n_shared + p->n_cls || l == p->num_layers - 1;
        if (L.cin < 4 || L.cin % 4 != 0 || L.cin > (l == 0 ? RM_MAXCIN : RM_MAXW) || (l > 0 && L.cin % 16 != 0)) return false;
        if (fin ? (L.cout_pad != 16 || L.cout != (l == p->num_layers - 1 ? 7 : 1) || L.relu) : (!rm_width_ok(L.cout) || L.cout_pad != L.cout)) return false;
        if (L.w_off != w || L.affine_off != a) return false;
        w += (int64_t)L.cin * L.cout_pad;
        a += 2 * L.cout_pad;
    }
    // every layer reads what the layer before it in its chain wrote
    const int last_shared = p->n_shared - 1;
    for (int l = 1; l < p->num_layers; ++l) {
        const int prev = (l == p->n_shared || l == p->n_shared + p->n_cls + 1) ? last_shared : l - 1;
        if (p->layer[l].cin != p->layer[prev].cout) return false;
    }
    return w == p->packed_elems && a == p->affine_elems;
}

}  // namespace s2d

using namespace s2d;

extern "C" int s2d_roi_mlp_supported(int cin, int n_shared, int s0, int s1, int n_cls, int c0, int c1, int n_reg, int r0, int r1, int num_class,
                                     int code_size) {
    return rm_supported(cin, n_shared, s0, s1, n_cls, c0, c1, n_reg, r0, r1, num_class, code_size) ? 1 : 0;
}

extern "C" int s2d_roi_mlp_plan_make(int cin, int n_shared, int s0, int s1, int n_cls, int c0, int c1, int n_reg, int r0, int r1, int num_class,
                                     int code_size, s2d_roi_mlp_plan *plan) {
    S2D_CHECK_ARG(plan, "roi_mlp_plan_make: null plan");
    if (!rm_supported(cin, n_shared, s0, s1, n_cls, c0, c1, n_reg, r0, r1, num_class, code_size)) {
        set_error("roi_mlp: unsupported shape (cin %d; shared %d: %d %d; cls %d: %d %d; reg %d: %d %d; %d classes, code size %d)", cin, n_shared, s0, s1,
                  n_cls, c0, c1, n_reg, r0, r1, num_class, code_size);
        return S2D_ERR_UNSUPPORTED;
    }
    memset(plan, 0, sizeof(*plan));
    plan->n_shared = n_shared, plan->n_cls = n_cls, plan->n_reg = n_reg;
    int n = 0, a = 0;
    int64_t w = 0;
    auto add = [&](int in, int out, int out_pad, int relu) {
        s2d_roi_mlp_layer &L = plan->layer[n++];
        L.cin = in, L.cout = out, L.cout_pad = out_pad, L.relu = relu, L.affine_off = a, L.w_off = w;
        w += (int64_t)in * out_pad;
        a += 2 * out_pad;
    };
    const int shared_w[2] = {s0, s1}, cls_w[2] = {c0, c1}, reg_w[2] = {r0, r1};
    int pre = cin;
    for (int i = 0; i < n_shared; ++i) add(pre, shared_w[i], shared_w[i], 1), pre = shared_w[i];
    const int shared_out = pre;
    for (int i = 0; i < n_cls; ++i) add(pre, cls_w[i], cls_w[i], 1), pre = cls_w[i];
    add(pre, 1, 16, 0);
    pre = shared_out;
    for (int i = 0; i < n_reg; ++i) add(pre, reg_w[i], reg_w[i], 1), pre = reg_w[i];
    add(pre, 7, 16, 0);
    plan->num_layers = n, plan->packed_elems = w, plan->affine_elems = a;
    return S2D_OK;
}

extern "C" int64_t s2d_roi_mlp_packed_elems(int cin, int n_shared, int s0, int s1, int n_cls, int c0, int c1, int n_reg, int r0, int r1, int num_class,
                                            int code_size) {
    s2d_roi_mlp_plan plan;
    return s2d_roi_mlp_plan_make(cin, n_shared, s0, s1, n_cls, c0, c1, n_reg, r0, r1, num_class, code_size, &plan) == S2D_OK ? plan.packed_elems : 0;
}

extern "C" int s2d_roi_mlp_pack(const s2d_roi_mlp_plan *plan, const float *const *weights, float *packed, s2d_stream_t stream) {
    S2D_CHECK_ARG(rm_plan_ok(plan), "roi_mlp_pack: not a plan of s2d_roi_mlp_plan_make");
    S2D_CHECK_ARG(weights && packed, "roi_mlp_pack: null argument");
    RmPackSrc src;
    memset(&src, 0, sizeof(src));
    for (int l = 0; l < plan->num_layers; ++l) {
        S2D_CHECK_ARG(weights[l], "roi_mlp_pack: null weight of layer %d", l);
        src.w[l] = weights[l];
    }
    hipLaunchKernelGGL(roi_mlp_pack_kernel, dim3((unsigned)ceil_div(plan->packed_elems, 256)), dim3(256), 0, (hipStream_t)stream, *plan, src, packed);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_roi_mlp_run(const s2d_roi_mlp_plan *plan, const float *feats, int64_t rows, const float *packed, const float *affine,
                               float *rcnn_cls, float *rcnn_reg, s2d_stream_t stream) {
    S2D_CHECK_ARG(rm_plan_ok(plan), "roi_mlp_run: not a plan of s2d_roi_mlp_plan_make");
    S2D_CHECK_ARG(rows >= 0 && ceil_div(rows, RM_ROWS) < (1ll << 31), "roi_mlp_run: %lld rows", (long long)rows);
    if (rows == 0) return S2D_OK;
    S2D_CHECK_ARG(feats && packed && affine && rcnn_cls && rcnn_reg, "roi_mlp_run: null argument");
    S2D_CHECK_ARG(((uintptr_t)feats & 15) == 0, "roi_mlp_run: feats must be 16-byte aligned");
    hipLaunchKernelGGL(roi_mlp_kernel, dim3((unsigned)ceil_div(rows, RM_ROWS)), dim3(256), 0, (hipStream_t)stream, *plan, feats, rows, packed, affine,
                       rcnn_cls, rcnn_reg);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
