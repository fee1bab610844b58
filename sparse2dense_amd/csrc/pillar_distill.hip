// Feature loss of the PointPillars distillation branch (det3d/torchie/trainer/trainer.py:749-762) in one pass per direction.
//
//   sa = P(F_S_a), da = P(F_D_a), sb = P(F_S_b), db = P(F_D_b)          P = max_pool2d(., 2, 2), floor mode
//   A = da > 0, Bm = db > 0
//   loss = 10 * [ mean_{~A}(sa-da)^2 + mean_A(sa-da)^2 + mean_Bm(sa-da)^2 + mean_Bm(sb-db)^2 + mean_{~Bm}(sb-db)^2 ]
// (the third term indexes the `a` maps with the `b` mask, as the reference does).  Nothing of the pooled resolution reaches memory:
// every 2x2 window is pooled in registers, forward into seven per-block sums (sum_A, sum_all, sum_Bm of (sa-da)^2; sum_Bm, sum_all of
// (sb-db)^2; nA; nB) that a one-wave kernel folds in double in a fixed order (no atomics: deterministic), backward into the gradient of
// the window's selected student element.  The selection is re-derived, not saved, by torch's rule: scan (0,0) (0,1) (1,0) (1,1), a later
// element replaces the current one only if it is strictly greater or NaN, so the first of tied elements wins.  The backward writes every
// element of both student gradients exactly once: the three other window elements and a dropped odd row / column get 0.
//
// Two kernels, each in a forward and a backward form, for fp32 or bf16 students and teachers:
//
// pd_tile_kernel: student channels_last, teacher planar (the benchmarked mode: bf16 NHWC neck maps against the fp32 canvases of
//   the pillar scatter).  A workgroup of four waves owns a strip of 32 pooled pixels of one pooled row, for all channels.
//   Phase 1: each wave takes one (map, channel) at a time; lanes 0-31 read the 64 elements of input row 2*ph under the strip and lanes
//   32-63 those of row 2*ph+1, 8 bytes per lane, i.e. two contiguous 256-byte runs per wave-instruction.  A lane pools its horizontal pair, one
//   shuffle brings the other row over, and lanes 0-31 store the pooled value to the LDS tile [map][pixel][channel] with a row of
//   c + 4 floats.  The four pad floats keep rows 16-byte aligned for phase 2 and put the 32 stores of one instruction on 8 banks
//   (4-way, 2x the conflict-free store time); the tile moves 4 bytes each way per 48 bytes the strip reads from HBM, so this does not bound.
//   Phase 2: thread = (pixel, group of 8 channels), group fastest, which is the student's memory order: 16-byte loads of the four
//   window positions of both student maps (bf16), two ds_read_b128 of the pooled teacher values.  Within one 16-lane read group the
//   c + 4 row length leaves some 16-byte slots shared by two lanes (2-way); a swizzle would remove that and is not worth its cost here.
// pd_any_kernel: every other layout pair through strides, one thread per pooled element in the student's memory order.  Planar maps of
//   even width move as 8-byte (fp32) pairs, so the all-planar fp32 parity mode reads and writes 512 contiguous bytes per wave-instruction.
#include "s2d_common.h"
#include <algorithm>

namespace s2d {
namespace {

constexpr int PD_BLOCKS = 2048;      // forward partial rows (upper bound of the forward grids)
constexpr int PD_SUMS = 7;
constexpr int PD_PIX = 32;           // pooled pixels per strip
constexpr int PD_MAX_TILE_C = 192;   // 2 * 32 * (192 + 4) * 4 B = 49 KiB of LDS

typedef __bf16 pd_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 pd_bf16x8 __attribute__((ext_vector_type(8)));

struct PdGeo {
    int n, c, h, w, ph, pw;
};
// element strides of one pair of maps
struct PdStride {
    int64_t n, c, y, x;
};
// go * (20/nA, 20/(N-nA), 20/nB) for the `a` maps, go * (20/nB, 20/(N-nB)) for the `b` maps
struct PdScale {
    float a_pos, a_neg, a_b, b_pos, b_neg;
};

__device__ __forceinline__ void pd_load2(const float *p, float &a, float &b) {
    const float2 v = *reinterpret_cast<const float2 *>(p);
    a = v.x; b = v.y;
}
__device__ __forceinline__ void pd_load2(const __bf16 *p, float &a, float &b) {
    const pd_bf16x2 v = *reinterpret_cast<const pd_bf16x2 *>(p);
    a = (float)v[0]; b = (float)v[1];
}
__device__ __forceinline__ void pd_store2(float *p, float a, float b) { *reinterpret_cast<float2 *>(p) = float2{a, b}; }
__device__ __forceinline__ void pd_store2(__bf16 *p, float a, float b) {
    pd_bf16x2 v;
    v[0] = (__bf16)a; v[1] = (__bf16)b;
    *reinterpret_cast<pd_bf16x2 *>(p) = v;
}
__device__ __forceinline__ void pd_load8(const float *p, float (&v)[8]) {
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void pd_load8(const __bf16 *p, float (&v)[8]) {
    const pd_bf16x8 a = *reinterpret_cast<const pd_bf16x8 *>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)a[e];
}
__device__ __forceinline__ void pd_store8(float *p, const float (&v)[8]) {
    reinterpret_cast<float4 *>(p)[0] = float4{v[0], v[1], v[2], v[3]};
    reinterpret_cast<float4 *>(p)[1] = float4{v[4], v[5], v[6], v[7]};
}
__device__ __forceinline__ void pd_store8(__bf16 *p, const float (&v)[8]) {
    pd_bf16x8 a;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = (__bf16)v[e];
    *reinterpret_cast<pd_bf16x8 *>(p) = a;
}

// torch's max_pool2d update rule (a later element wins only if strictly greater or NaN)
__device__ __forceinline__ bool pd_takes(float v, float m) { return v > m || v != v; }

// window in scan order (0,0) (0,1) (1,0) (1,1) -> selected position and its value
__device__ __forceinline__ int pd_select(const float (&v)[4], float &m) {
    int k = 0;
    m = v[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (pd_takes(v[j], m)) {
            m = v[j];
            k = j;
        }
    return k;
}

__device__ __forceinline__ void pd_accum(float sa, float da, float sb, float db, float (&acc)[PD_SUMS]) {
    const float d = sa - da, d2 = d * d, e = sb - db, e2 = e * e;
    const bool A = da > 0.f, B = db > 0.f;
    acc[0] += A ? d2 : 0.f;
    acc[1] += d2;
    acc[2] += B ? d2 : 0.f;
    acc[3] += B ? e2 : 0.f;
    acc[4] += e2;
    acc[5] += A ? 1.f : 0.f;
    acc[6] += B ? 1.f : 0.f;
}

// selects, not products with 0/1: the scale of an empty class is infinite and must not reach an element outside it
__device__ __forceinline__ float pd_grad_a(float sa, float da, float db, const PdScale &k) {
    return (sa - da) * ((da > 0.f ? k.a_pos : k.a_neg) + (db > 0.f ? k.a_b : 0.f));
}
__device__ __forceinline__ float pd_grad_b(float sb, float db, const PdScale &k) { return (sb - db) * (db > 0.f ? k.b_pos : k.b_neg); }

__device__ __forceinline__ PdScale pd_scales(const float *__restrict__ out8, const float *__restrict__ go) {
    const float g = go[0];
    return PdScale{g * out8[1], g * out8[2], g * out8[3], g * out8[4], g * out8[5]};
}

// block-wide sums of PD_SUMS floats per thread -> out[blockIdx][PD_SUMS]: lanes by shuffles, then the four waves in order
__device__ __forceinline__ void pd_block_sums(float (&v)[PD_SUMS], float *__restrict__ out) {
    __shared__ float red[4][PD_SUMS];
#pragma unroll
    for (int k = 0; k < PD_SUMS; ++k) {
        float s = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < PD_SUMS)
        out[(int64_t)blockIdx.x * PD_SUMS + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

template <typename T>
__device__ __forceinline__ void pd_load_win(const T *__restrict__ p, const PdStride &s, bool pair, float (&v)[4]) {
    if (pair) {
        pd_load2(p, v[0], v[1]);
        pd_load2(p + s.y, v[2], v[3]);
    } else {
        v[0] = (float)p[0]; v[1] = (float)p[s.x]; v[2] = (float)p[s.y]; v[3] = (float)p[s.y + s.x];
    }
}

// the gradient g at window position k, zeros at the other three and at a dropped column / row behind the last window
template <typename T>
__device__ __forceinline__ void pd_store_win(T *__restrict__ p, const PdStride &s, bool pair, int k, float g, bool last_x, bool last_y) {
    const float o0 = k == 0 ? g : 0.f, o1 = k == 1 ? g : 0.f, o2 = k == 2 ? g : 0.f, o3 = k == 3 ? g : 0.f;
    if (pair) {
        pd_store2(p, o0, o1);
        pd_store2(p + s.y, o2, o3);
    } else {
        p[0] = (T)o0; p[s.x] = (T)o1; p[s.y] = (T)o2; p[s.y + s.x] = (T)o3;
    }
    if (last_x) {
        p[2 * s.x] = (T)0.f; p[s.y + 2 * s.x] = (T)0.f;
    }
    if (last_y) {
        p[2 * s.y] = (T)0.f; p[2 * s.y + s.x] = (T)0.f;
        if (last_x) p[2 * s.y + 2 * s.x] = (T)0.f;
    }
}

// any layout pair: one thread per pooled element, enumerated in the student's memory order (s_nhwc: channel fastest)
template <typename TS, typename TT, bool BWD>
__global__ __launch_bounds__(256) void pd_any_kernel(const TS *__restrict__ sa, const TS *__restrict__ sb, const TT *__restrict__ da,
                                                     const TT *__restrict__ db, PdGeo g, PdStride ss, PdStride ts, int s_nhwc, int s_pair,
                                                     int t_pair, float *__restrict__ partial, const float *__restrict__ out8,
                                                     const float *__restrict__ go, TS *__restrict__ dsa, TS *__restrict__ dsb) {
    float acc[PD_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    PdScale k = {};
    if (BWD) k = pd_scales(out8, go);
    const bool odd_w = g.w & 1, odd_h = g.h & 1;
    const int64_t total = (int64_t)g.n * g.c * g.ph * g.pw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int n, ch, py, px;
        int64_t r = i;
        if (s_nhwc) {
            ch = (int)(r % g.c); r /= g.c;
            px = (int)(r % g.pw); r /= g.pw;
            py = (int)(r % g.ph); n = (int)(r / g.ph);
        } else {
            px = (int)(r % g.pw); r /= g.pw;
            py = (int)(r % g.ph); r /= g.ph;
            ch = (int)(r % g.c); n = (int)(r / g.c);
        }
        const int64_t so = n * ss.n + ch * ss.c + 2 * py * ss.y + 2 * px * ss.x;
        const int64_t to = n * ts.n + ch * ts.c + 2 * py * ts.y + 2 * px * ts.x;
        float va[4], vb[4], wa[4], wb[4], ma, mb, ta, tb;
        pd_load_win(sa + so, ss, s_pair, va);
        pd_load_win(sb + so, ss, s_pair, vb);
        pd_load_win(da + to, ts, t_pair, wa);
        pd_load_win(db + to, ts, t_pair, wb);
        const int ka = pd_select(va, ma), kb = pd_select(vb, mb);
        pd_select(wa, ta);
        pd_select(wb, tb);
        if (BWD) {
            const bool lx = odd_w && px == g.pw - 1, ly = odd_h && py == g.ph - 1;
            pd_store_win(dsa + so, ss, s_pair, ka, pd_grad_a(ma, ta, tb, k), lx, ly);
            pd_store_win(dsb + so, ss, s_pair, kb, pd_grad_b(mb, tb, k), lx, ly);
        } else {
            pd_accum(ma, ta, mb, tb, acc);
        }
    }
    if (!BWD) pd_block_sums(acc, partial);
}

// student channels_last, teacher planar, c <= PD_MAX_TILE_C: strips of PD_PIX pooled pixels (file header).  tile: 2 * PD_PIX * (c + 4) floats.
template <typename TS, typename TT, bool BWD>
__global__ __launch_bounds__(256) void pd_tile_kernel(const TS *__restrict__ sa, const TS *__restrict__ sb, const TT *__restrict__ da,
                                                      const TT *__restrict__ db, PdGeo g, int64_t strips, int strips_per_row, int t_pair,
                                                      float *__restrict__ partial, const float *__restrict__ out8, const float *__restrict__ go,
                                                      TS *__restrict__ dsa, TS *__restrict__ dsb) {
    extern __shared__ __attribute__((aligned(16))) float pd_tile[];
    const int ld = g.c + 4, groups = g.c >> 3;
    const int t = threadIdx.x, wave = t >> 6, half = (t >> 5) & 1, pl = t & 31;
    float acc[PD_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    PdScale k = {};
    if (BWD) k = pd_scales(out8, go);
    const bool odd_w = g.w & 1, odd_h = g.h & 1;
    const int64_t sx = g.c, sy = (int64_t)g.w * g.c;
    for (int64_t s = blockIdx.x; s < strips; s += gridDim.x) {
        const int p0 = (int)(s % strips_per_row) * PD_PIX;
        const int64_t row = s / strips_per_row;
        const int py = (int)(row % g.ph), n = (int)(row / g.ph);
        const int npix = min(PD_PIX, g.pw - p0);
        // phase 1: pooled teacher values of the strip -> tile[map][pixel][channel]
        // a wave takes the (map, channel) units wave, wave + 4, ...: c / 2 of them, four at a time (c % 8 == 0) so that four loads are in flight
        for (int ub = wave; ub < 2 * g.c; ub += 16) {
            float mine[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int u = ub + 4 * j, m = u >= g.c ? 1 : 0, ch = u - m * g.c;
                const TT *src = (m ? db : da) + ((((int64_t)n * g.c + ch) * g.h + 2 * py + half) * g.w + 2 * (p0 + pl));
                float v0 = 0.f, v1 = 0.f;
                if (pl < npix) {
                    if (t_pair) {
                        pd_load2(src, v0, v1);
                    } else {
                        v0 = (float)src[0]; v1 = (float)src[1];
                    }
                }
                mine[j] = pd_takes(v1, v0) ? v1 : v0;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int u = ub + 4 * j, m = u >= g.c ? 1 : 0, ch = u - m * g.c;
                const float other = __shfl_xor(mine[j], 32, 64);   // lanes 0-31 hold input row 2*py, lanes 32-63 row 2*py + 1
                if (half == 0 && pl < npix) pd_tile[(m * PD_PIX + pl) * ld + ch] = pd_takes(other, mine[j]) ? other : mine[j];
            }
        }
        __syncthreads();
        // phase 2: the student's windows, 8 channels per thread
        for (int it = t; it < npix * groups; it += 256) {
            const int pix = it / groups, grp = it - pix * groups;
            const int64_t off = (((int64_t)n * g.h + 2 * py) * g.w + 2 * (p0 + pix)) * g.c + 8 * grp;
            float a[4][8], b[4][8], ta[8], tb[8];
            pd_load8(sa + off, a[0]); pd_load8(sa + off + sx, a[1]); pd_load8(sa + off + sy, a[2]); pd_load8(sa + off + sy + sx, a[3]);
            pd_load8(sb + off, b[0]); pd_load8(sb + off + sx, b[1]); pd_load8(sb + off + sy, b[2]); pd_load8(sb + off + sy + sx, b[3]);
            pd_load8(pd_tile + pix * ld + 8 * grp, ta);
            pd_load8(pd_tile + (PD_PIX + pix) * ld + 8 * grp, tb);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float va[4] = {a[0][e], a[1][e], a[2][e], a[3][e]}, vb[4] = {b[0][e], b[1][e], b[2][e], b[3][e]};
                float ma, mb;
                const int ka = pd_select(va, ma), kb = pd_select(vb, mb);
                if (BWD) {
                    const float ga = pd_grad_a(ma, ta[e], tb[e], k), gb = pd_grad_b(mb, tb[e], k);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        a[j][e] = j == ka ? ga : 0.f;
                        b[j][e] = j == kb ? gb : 0.f;
                    }
                } else {
                    pd_accum(ma, ta[e], mb, tb[e], acc);
                }
            }
            if (BWD) {
                pd_store8(dsa + off, a[0]); pd_store8(dsa + off + sx, a[1]); pd_store8(dsa + off + sy, a[2]); pd_store8(dsa + off + sy + sx, a[3]);
                pd_store8(dsb + off, b[0]); pd_store8(dsb + off + sx, b[1]); pd_store8(dsb + off + sy, b[2]); pd_store8(dsb + off + sy + sx, b[3]);
                const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                const bool lx = odd_w && p0 + pix == g.pw - 1, ly = odd_h && py == g.ph - 1;
                if (lx) {
                    pd_store8(dsa + off + 2 * sx, z); pd_store8(dsa + off + sy + 2 * sx, z);
                    pd_store8(dsb + off + 2 * sx, z); pd_store8(dsb + off + sy + 2 * sx, z);
                }
                if (ly) {
                    pd_store8(dsa + off + 2 * sy, z); pd_store8(dsa + off + 2 * sy + sx, z);
                    pd_store8(dsb + off + 2 * sy, z); pd_store8(dsb + off + 2 * sy + sx, z);
                    if (lx) {
                        pd_store8(dsa + off + 2 * sy + 2 * sx, z);
                        pd_store8(dsb + off + 2 * sy + 2 * sx, z);
                    }
                }
            }
        }
        __syncthreads();   // the next strip overwrites the tile
    }
    if (!BWD) pd_block_sums(acc, partial);
}

// out[0] = loss, out[1..5] = 20/nA, 20/(N-nA), 20/nB (`a` maps), 20/nB, 20/(N-nB) (`b` maps), out[6] = nA, out[7] = nB
__global__ __launch_bounds__(64) void pd_finalize_kernel(const float *__restrict__ partial, int nb, double n, float *__restrict__ out) {
    double v[PD_SUMS] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < nb; i += 64)
        for (int k = 0; k < PD_SUMS; ++k) v[k] += partial[i * PD_SUMS + k];
#pragma unroll
    for (int k = 0; k < PD_SUMS; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    if (threadIdx.x != 0) return;
    const double nA = v[5], nB = v[6];
    // an empty class gives nan, as torch's mean of nothing
    out[0] = (float)(10.0 * ((v[1] - v[0]) / (n - nA) + v[0] / nA + v[2] / nB + v[3] / nB + (v[4] - v[3]) / (n - nB)));
    out[1] = (float)(20.0 / nA);
    out[2] = (float)(20.0 / (n - nA));
    out[3] = (float)(20.0 / nB);
    out[4] = (float)(20.0 / nB);
    out[5] = (float)(20.0 / (n - nB));
    out[6] = (float)nA;
    out[7] = (float)nB;
}

PdStride pd_strides(int nhwc, int c, int h, int w) {
    if (nhwc) return PdStride{(int64_t)h * w * c, 1, (int64_t)w * c, c};
    return PdStride{(int64_t)c * h * w, (int64_t)h * w, w, 1};
}

int pd_check(const char *who, const void *sa, const void *sb, const void *da, const void *db, int n, int c, int h, int w) {
    S2D_CHECK_ARG(sa && sb && da && db && n > 0 && c > 0 && h > 0 && w > 0, "%s: bad argument", who);
    if (c % 8 || h < 2 || w < 2) {
        set_error("%s: needs c %% 8 == 0, h >= 2 and w >= 2 (c=%d h=%d w=%d)", who, c, h, w);
        return S2D_ERR_UNSUPPORTED;
    }
    if (((uintptr_t)sa | (uintptr_t)sb | (uintptr_t)da | (uintptr_t)db) & 15) {
        set_error("%s: the maps must be 16-byte aligned", who);
        return S2D_ERR_UNSUPPORTED;
    }
    return S2D_OK;
}

template <typename TS, typename TT, bool BWD>
void pd_launch(const void *sa, const void *sb, int s_nhwc, const void *da, const void *db, int t_nhwc, int n, int c, int h, int w, float *partial,
               int *blocks, const float *out8, const float *go, void *dsa, void *dsb, hipStream_t st) {
    const PdGeo g{n, c, h, w, h / 2, w / 2};
    const int planar_pair = (w & 1) == 0;   // rows of a planar map start on an even element: 2-element accesses are aligned
    if (s_nhwc && !t_nhwc && c <= PD_MAX_TILE_C) {
        const int spr = (int)ceil_div(g.pw, PD_PIX);
        const int64_t strips = (int64_t)n * g.ph * spr;
        const int nb = (int)std::min<int64_t>(strips, BWD ? 16 * PD_BLOCKS : PD_BLOCKS);
        const size_t lds = (size_t)2 * PD_PIX * (c + 4) * sizeof(float);
        hipLaunchKernelGGL((pd_tile_kernel<TS, TT, BWD>), dim3(nb), dim3(256), lds, st, (const TS *)sa, (const TS *)sb, (const TT *)da,
                           (const TT *)db, g, strips, spr, planar_pair, partial, out8, go, (TS *)dsa, (TS *)dsb);
        *blocks = nb;
        return;
    }
    const int64_t total = (int64_t)n * c * g.ph * g.pw;
    const int nb = (int)std::min<int64_t>(ceil_div(total, 256), BWD ? 32 * PD_BLOCKS : PD_BLOCKS);
    hipLaunchKernelGGL((pd_any_kernel<TS, TT, BWD>), dim3(nb), dim3(256), 0, st, (const TS *)sa, (const TS *)sb, (const TT *)da, (const TT *)db, g,
                       pd_strides(s_nhwc, c, h, w), pd_strides(t_nhwc, c, h, w), s_nhwc, !s_nhwc && planar_pair, !t_nhwc && planar_pair, partial,
                       out8, go, (TS *)dsa, (TS *)dsb);
    *blocks = nb;
}

template <bool BWD>
void pd_dispatch(const void *sa, const void *sb, int s_bf16, int s_nhwc, const void *da, const void *db, int t_bf16, int t_nhwc, int n, int c, int h,
                 int w, float *partial, int *blocks, const float *out8, const float *go, void *dsa, void *dsb, hipStream_t st) {
#define S2D_PD(TS, TT) pd_launch<TS, TT, BWD>(sa, sb, s_nhwc, da, db, t_nhwc, n, c, h, w, partial, blocks, out8, go, dsa, dsb, st)
    if (s_bf16 && t_bf16) S2D_PD(__bf16, __bf16);
    else if (s_bf16) S2D_PD(__bf16, float);
    else if (t_bf16) S2D_PD(float, __bf16);
    else S2D_PD(float, float);
#undef S2D_PD
}

}  // namespace
}  // namespace s2d

using namespace s2d;

extern "C" size_t s2d_pooled_distill_workspace_bytes(void) { return (size_t)PD_BLOCKS * PD_SUMS * sizeof(float) + 256; }

// sa, sb: the student's maps [n, c, h, w], one element type (student_bf16) and one memory order (student_nhwc: channels_last, else
// planar); da, db: the teacher's, likewise.  out8 (device): loss, five gradient scales, nA, nB.
extern "C" int s2d_pooled_distill_fwd(const void *sa, const void *sb, int student_bf16, int student_nhwc, const void *da, const void *db,
                                      int teacher_bf16, int teacher_nhwc, int n, int c, int h, int w, float *out8, void *ws, size_t ws_bytes,
                                      s2d_stream_t stream) {
    const int rc = pd_check("pooled_distill_fwd", sa, sb, da, db, n, c, h, w);
    if (rc != S2D_OK) return rc;
    S2D_CHECK_ARG(out8, "pooled_distill_fwd: bad argument");
    if (!ws || ws_bytes < s2d_pooled_distill_workspace_bytes()) {
        set_error("pooled_distill_fwd: workspace too small");
        return S2D_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    float *partial = (float *)ws;
    int nb = 0;
    pd_dispatch<false>(sa, sb, student_bf16, student_nhwc, da, db, teacher_bf16, teacher_nhwc, n, c, h, w, partial, &nb, nullptr, nullptr, nullptr,
                       nullptr, st);
    S2D_LAUNCH_CHECK();
    hipLaunchKernelGGL(pd_finalize_kernel, dim3(1), dim3(64), 0, st, partial, nb, (double)n * c * (h / 2) * (w / 2), out8);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

// dsa, dsb (the student's element type and memory order) = go * d loss / d student map; every element is written
extern "C" int s2d_pooled_distill_bwd(const void *sa, const void *sb, int student_bf16, int student_nhwc, const void *da, const void *db,
                                      int teacher_bf16, int teacher_nhwc, int n, int c, int h, int w, const float *out8, const float *go,
                                      void *dsa, void *dsb, s2d_stream_t stream) {
    const int rc = pd_check("pooled_distill_bwd", sa, sb, da, db, n, c, h, w);
    if (rc != S2D_OK) return rc;
    S2D_CHECK_ARG(out8 && go && dsa && dsb, "pooled_distill_bwd: bad argument");
    if (((uintptr_t)dsa | (uintptr_t)dsb) & 15) {
        set_error("pooled_distill_bwd: the gradient maps must be 16-byte aligned");
        return S2D_ERR_UNSUPPORTED;
    }
    int nb = 0;
    pd_dispatch<true>(sa, sb, student_bf16, student_nhwc, da, db, teacher_bf16, teacher_nhwc, n, c, h, w, nullptr, &nb, out8, go, dsa, dsb,
                      (hipStream_t)stream);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
