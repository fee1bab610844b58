// Deformable convolution v1 (det3d/ops/dcn: DeformConvFunction over deform_conv_cuda_kernel.cu's im2col + GEMM) as fused implicit
// GEMMs on v_mfma_f32_16x16x32_bf16: the bilinear gather feeds the LDS operand tile directly, no column buffer exists in global memory.
//   x, y, dy, dx   bf16 NHWC;   offset / d_offset  fp32 or bf16 NHWC [n][ho][wo][dg * 2 * kh * kw]  (channel g*2*K + 2*tap: row offset,
//   + 1: column offset - the reference's channel order, channels_last);   weight fp32 [cout][cin][kh][kw], packed once per change.
// Sampling (deformable_im2col_bilinear): position h = ho*stride - pad + i*dil + off_h (w alike); the value is 0 unless
// h > -1 && w > -1 && h < H && w < W (all strict; NaN fails every comparison), else the bilinear blend of the corners
// (floor, floor + 1), each corner counted only inside [0, H-1] x [0, W-1].  The window test comes BEFORE the float -> int conversion
// and every corner index is clamped into the map before it forms an address: +-1e6, NaN and Inf offsets touch nothing outside x / dx.
//
// A workgroup is 256 threads on 64 output pixels.  In the gather role thread t serves pixel t / 4 and the 16-channel segment t % 4 of
// the current 64-channel chunk: it reads the tap's two offsets of its deformable group, forms the four corner weights and masks in
// fp32, gathers 4 x 32 bytes (the four lanes of a pixel read 128 contiguous bytes per corner), blends in fp32 and writes 16 bf16
// into the [64 px][64 ch] LDS tile (16-byte parts XOR-swizzled by row & 7, as conv2d_nhwc.hip does).
//   fwd    K-step = (tap, chunk); wave v owns 64 px x 16 couts (4 accumulators); B fragments come pre-laid from the packed weight
//          (L2 resident: 72 KB at 64 -> 64); the next step's gather is in flight while the MFMAs of this one run (two LDS tiles).
//   dgrad  dcol = dY * W^T per (tap, chunk) on the MFMA (dY tile staged once, ReLU mask re-derived from the saved output), through an
//          fp32 LDS tile back to the gather role: d_offset = the 16-channel reduction of dcol * d(sample)/d(position) (one owner per
//          element, written directly), dX = fp32 atomic adds of weight * dcol to the four corners of an fp32 image, converted to bf16
//          by a second kernel.
//   wgrad  per workgroup (pixel range, tap, cin chunk, cout block): col^T * dY with both operands transposed through LDS; fp32
//          partials per workgroup, folded in a fixed order by a reduce kernel (no atomics: bit-identical from run to run).
// Written for: groups 1, cin and cout multiples of 64 up to 256, cin / dg in {16, 32, 64}, kernel extents up to 7, any stride / padding /
// dilation.  ENABLED (s2d_deform_conv_supported) only for the shape the GPU suite runs: 64 -> 64, 3x3, stride 1, padding 1, dilation 1, dg 4.
#include <algorithm>

#include "s2d_common.h"

namespace s2d {

typedef float f32x4d __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8d __attribute__((ext_vector_type(8)));

constexpr int DCN_MAX_C = 256;

struct DcnGeo {
    int n_img, H, W, cin, cout, kh, kw, stride, pad, dil, dg, Ho, Wo;
};

// The shapes the GPU suite runs the kernels at (tests/test_deform_conv_gpu.py) - the deformable conv of the nuScenes head: 64 -> 64, 3x3,
// stride 1, padding 1, dilation 1, 4 deformable groups of 16 channels.  The kernels are written for the wider family below
// (dcn_kernel_family); a shape joins `supported` together with a GPU comparison against the float64 composite, not before.
static bool dcn_kernel_family(int cin, int cout, int kh, int kw, int stride, int pad, int dil, int groups, int dg) {
    if (groups != 1 || dg < 1 || kh < 1 || kw < 1 || kh > 7 || kw > 7 || stride < 1 || pad < 0 || dil < 1) return false;
    if (cin < 64 || cout < 64 || cin % 64 || cout % 64 || cin > DCN_MAX_C || cout > DCN_MAX_C || cin % dg) return false;
    const int cg = cin / dg;
    return cg == 16 || cg == 32 || cg == 64;
}
static bool dcn_supported(int cin, int cout, int kh, int kw, int stride, int pad, int dil, int groups, int dg) {
    return dcn_kernel_family(cin, cout, kh, kw, stride, pad, dil, groups, dg) && cin == 64 && cout == 64 && kh == 3 && kw == 3 && stride == 1 &&
           pad == 1 && dil == 1 && dg == 4;
}

// CUs of the CURRENT device, asked every time (a host query of microseconds per weight-gradient launch): a cached value would belong to
// whichever device was current first
static int dcn_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
}

// ---- sampling --------------------------------------------------------------------------------------------------------------------
struct DcnSample {
    float w[4];     // corner weights hh*hw, hh*lw, lh*hw, lh*lw (unmasked)
    float lh, lw;
    int pix[4];     // y * W + x of the clamped corners: always inside the map
    bool ok[4];     // corner counted (position inside the window and corner inside the map)
};

__device__ __forceinline__ DcnSample dcn_sample(float h, float w, int H, int W) {
    DcnSample s;
    const bool inside = h > -1.f && w > -1.f && h < (float)H && w < (float)W;   // false for NaN
    const float hs = inside ? h : 0.f, ws = inside ? w : 0.f;                    // only in-window values reach the conversion
    const float fh = floorf(hs), fw = floorf(ws);
    const int hl = (int)fh, wl = (int)fw;                                        // in [-1, H-1] x [-1, W-1]
    s.lh = hs - fh;
    s.lw = ws - fw;
    const float hh = 1.f - s.lh, hw = 1.f - s.lw;
    const bool t = inside && hl >= 0, b = inside && hl + 1 <= H - 1, l = inside && wl >= 0, r = inside && wl + 1 <= W - 1;
    const int y0 = hl < 0 ? 0 : hl, y1 = hl + 1 > H - 1 ? H - 1 : hl + 1;
    const int x0 = wl < 0 ? 0 : wl, x1 = wl + 1 > W - 1 ? W - 1 : wl + 1;
    s.w[0] = hh * hw; s.w[1] = hh * s.lw; s.w[2] = s.lh * hw; s.w[3] = s.lh * s.lw;
    s.pix[0] = y0 * W + x0; s.pix[1] = y0 * W + x1; s.pix[2] = y1 * W + x0; s.pix[3] = y1 * W + x1;
    s.ok[0] = t && l; s.ok[1] = t && r; s.ok[2] = b && l; s.ok[3] = b && r;
    return s;
}

__device__ __forceinline__ float dcn_ld(const float *p) { return *p; }
__device__ __forceinline__ float dcn_ld(const __bf16 *p) { return (float)*p; }
__device__ __forceinline__ void dcn_st(float *p, float v) { *p = v; }
__device__ __forceinline__ void dcn_st(__bf16 *p, float v) { *p = (__bf16)v; }

// the gather role of a thread: pixel, segment, and where its pixel sits
struct DcnRole {
    int p, seg, img, ho, wo;
    bool live;
    int64_t m;
};
__device__ __forceinline__ DcnRole dcn_role(int64_t m0, int64_t m_total, const DcnGeo &g) {
    DcnRole r;
    r.p = threadIdx.x >> 2;
    r.seg = threadIdx.x & 3;
    const int64_t m = m0 + r.p;
    r.live = m < m_total;
    r.m = r.live ? m : 0;
    r.wo = (int)(r.m % g.Wo);
    r.ho = (int)((r.m / g.Wo) % g.Ho);
    r.img = (int)(r.m / ((int64_t)g.Wo * g.Ho));
    return r;
}

template <typename OT>
__device__ __forceinline__ DcnSample dcn_tap_sample(const OT *off, const DcnRole &r, const DcnGeo &g, int tap, int grp) {
    const int taps = g.kh * g.kw;
    const OT *o = off + r.m * (int64_t)(g.dg * 2 * taps) + grp * 2 * taps + 2 * tap;
    const float oh = dcn_ld(o), ow = dcn_ld(o + 1);
    const int i = tap / g.kw, j = tap - i * g.kw;
    return dcn_sample((float)(r.ho * g.stride - g.pad + i * g.dil) + oh, (float)(r.wo * g.stride - g.pad + j * g.dil) + ow, g.H, g.W);
}

// the four corners' 16 channels; corners that do not count read nothing and hold zeros
__device__ __forceinline__ void dcn_gather(const __bf16 *__restrict__ x, const DcnSample &s, const DcnRole &r, const DcnGeo &g, int c0,
                                           bf16x8d (&v)[4][2]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k][0] = bf16x8d{};
        v[k][1] = bf16x8d{};
        if (s.ok[k] && r.live) {
            const bf16x8d *src = reinterpret_cast<const bf16x8d *>(x + ((int64_t)r.img * g.H * g.W + s.pix[k]) * g.cin + c0);
            v[k][0] = src[0];
            v[k][1] = src[1];
        }
    }
}

__device__ __forceinline__ void dcn_blend(const DcnSample &s, const bf16x8d (&v)[4][2], bf16x8d (&out)[2]) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float val = s.w[0] * (float)v[0][hf][e] + s.w[1] * (float)v[1][hf][e] + s.w[2] * (float)v[2][hf][e] + s.w[3] * (float)v[3][hf][e];
            out[hf][e] = (__bf16)val;
        }
}

// 16-byte part `part` of row `row` in a swizzled [64][64 bf16] tile
__device__ __forceinline__ char *dcn_tile_at(char *tile, int row, int part) { return tile + (row * 8 + (part ^ (row & 7))) * 16; }

// ---- weight images -----------------------------------------------------------------------------------------------------------------
// fwd  [tap][chunk][cout/16][2][64 lanes][8]: B fragment of K-half hf: cout nt*16 + (lane & 15), cin chunk*64 + hf*32 + (lane >> 4)*8 + e
// bwd  [tap][chunk][4][cout/32][64 lanes][8]: B fragment of W^T:       cin chunk*64 + nt*16 + (lane & 15), cout ks*32 + (lane >> 4)*8 + e
__global__ __launch_bounds__(256) void dcn_pack_kernel(const float *__restrict__ w, int cin, int cout, int taps, __bf16 *__restrict__ pf,
                                                       __bf16 *__restrict__ pb) {
    const int64_t total = (int64_t)taps * cin * cout;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int chunks = cin / 64;
    const int e = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
    int64_t rest = idx >> 9;
    {
        const int hf = (int)(rest & 1);
        int64_t t = rest >> 1;
        const int nt = (int)(t % (cout / 16));
        t /= cout / 16;
        const int chunk = (int)(t % chunks), tap = (int)(t / chunks);
        const int co = nt * 16 + (lane & 15), c = chunk * 64 + hf * 32 + (lane >> 4) * 8 + e;
        pf[idx] = (__bf16)w[((int64_t)co * cin + c) * taps + tap];
    }
    {
        const int ks = (int)(rest % (cout / 32));
        int64_t t = rest / (cout / 32);
        const int nt = (int)(t & 3);
        t >>= 2;
        const int chunk = (int)(t % chunks), tap = (int)(t / chunks);
        const int c = chunk * 64 + nt * 16 + (lane & 15), co = ks * 32 + (lane >> 4) * 8 + e;
        pb[idx] = (__bf16)w[((int64_t)co * cin + c) * taps + tap];
    }
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <typename OT>
__global__ __launch_bounds__(256) void dcn_fwd_kernel(const __bf16 *__restrict__ x, const OT *__restrict__ off, const __bf16 *__restrict__ wpack,
                                                      DcnGeo g, int relu, __bf16 *__restrict__ y) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 8192];
    const int64_t m_total = (int64_t)g.n_img * g.Ho * g.Wo;
    const int64_t m0 = (int64_t)xcd_tile(blockIdx.x, gridDim.x) * 64;
    if (m0 >= m_total) return;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int blk_n = blockIdx.y;
    const int chunks = g.cin / 64, taps = g.kh * g.kw, ksteps = taps * chunks, cg = g.cin / g.dg, ntiles = g.cout / 16;
    const DcnRole role = dcn_role(m0, m_total, g);

    DcnSample smp;
    bf16x8d v[4][2];
    auto fetch = [&](int s) {
        const int tap = s / chunks, chunk = s - tap * chunks;
        const int c0 = chunk * 64 + role.seg * 16;
        smp = dcn_tap_sample(off, role, g, tap, c0 / cg);
        dcn_gather(x, smp, role, g, c0, v);
    };
    auto put = [&](int buf) {
        bf16x8d o[2];
        dcn_blend(smp, v, o);
        char *tile = smem + buf * 8192;
        *reinterpret_cast<bf16x8d *>(dcn_tile_at(tile, role.p, 2 * role.seg)) = o[0];
        *reinterpret_cast<bf16x8d *>(dcn_tile_at(tile, role.p, 2 * role.seg + 1)) = o[1];
    };

    f32x4d acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4d{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    put(0);
    __syncthreads();
    for (int s = 0; s < ksteps; ++s) {
        const int cur = s & 1;
        if (s + 1 < ksteps) fetch(s + 1);   // in flight across the MFMAs below
        const char *tile = smem + cur * 8192;
        const bf16x8d *bsrc = reinterpret_cast<const bf16x8d *>(wpack) + (((int64_t)s * ntiles + blk_n * 4 + wid) * 2) * 64 + lane;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const bf16x8d b = bsrc[hf * 64];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bf16x8d a = *reinterpret_cast<const bf16x8d *>(dcn_tile_at(const_cast<char *>(tile), 16 * i + r, 4 * hf + q));
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i], 0, 0, 0);
            }
        }
        if (s + 1 < ksteps) put(cur ^ 1);   // last read in step s - 1, behind that step's barrier
        __syncthreads();
    }

    // C layout: pixel 16 i + 4 q + reg, cout wid*16 + r -> plain [64 px][64 couts] bf16 in LDS -> 2 x 16-byte stores per thread
    __bf16 *stage = reinterpret_cast<__bf16 *>(smem);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float val = acc[i][e];
            if (relu) val = val > 0.f ? val : 0.f;
            stage[(16 * i + 4 * q + e) * 64 + wid * 16 + r] = (__bf16)val;
        }
    __syncthreads();
    if (role.live) {
        const bf16x8d *src = reinterpret_cast<const bf16x8d *>(stage + role.p * 64 + role.seg * 16);
        bf16x8d *dst = reinterpret_cast<bf16x8d *>(y + role.m * g.cout + blk_n * 64 + role.seg * 16);
        dst[0] = src[0];
        dst[1] = src[1];
    }
}

// dY of the tile (x the ReLU mask of the saved output), 16 couts at c0, as two 16-byte vectors; dead pixels give zeros
__device__ __forceinline__ void dcn_load_dy(const __bf16 *__restrict__ dy, const __bf16 *__restrict__ ysaved, const DcnRole &r, int cout, int c0,
                                            bf16x8d (&d)[2]) {
    d[0] = bf16x8d{};
    d[1] = bf16x8d{};
    if (!r.live) return;
    const bf16x8d *src = reinterpret_cast<const bf16x8d *>(dy + r.m * cout + c0);
    d[0] = src[0];
    d[1] = src[1];
    if (ysaved) {
        const bf16x8d *ys = reinterpret_cast<const bf16x8d *>(ysaved + r.m * cout + c0);
        const bf16x8d y0 = ys[0], y1 = ys[1];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (!((float)y0[e] > 0.f)) d[0][e] = (__bf16)0.f;
            if (!((float)y1[e] > 0.f)) d[1][e] = (__bf16)0.f;
        }
    }
}

// ---- data backward: dX (fp32 image, atomics) and d_offset (direct) ---------------------------------------------------------------
constexpr int DCN_DCOL_LD = 68;   // fp32 row pitch of the dcol tile

template <typename OT>
__global__ __launch_bounds__(256) void dcn_bwd_data_kernel(const __bf16 *__restrict__ x, const OT *__restrict__ off, const __bf16 *__restrict__ dy,
                                                           const __bf16 *__restrict__ ysaved, const __bf16 *__restrict__ wpack_t, DcnGeo g,
                                                           float *__restrict__ dx32, OT *__restrict__ doff) {
    extern __shared__ __attribute__((aligned(16))) char dys[];   // dY tile: one swizzled [64][64] image (8 KiB) per 64 couts
    __shared__ __attribute__((aligned(16))) float dcol[64 * DCN_DCOL_LD];
    const int64_t m_total = (int64_t)g.n_img * g.Ho * g.Wo;
    const int64_t m0 = (int64_t)xcd_tile(blockIdx.x, gridDim.x) * 64;
    if (m0 >= m_total) return;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int chunks = g.cin / 64, taps = g.kh * g.kw, cg = g.cin / g.dg, kchunks = g.cout / 64, ksl = g.cout / 32;
    const int lpg = cg / 16;   // lanes (segments) that share a deformable group: 1, 2 or 4
    const DcnRole role = dcn_role(m0, m_total, g);

    for (int kc = 0; kc < kchunks; ++kc) {
        bf16x8d d[2];
        dcn_load_dy(dy, ysaved, role, g.cout, kc * 64 + role.seg * 16, d);
        *reinterpret_cast<bf16x8d *>(dcn_tile_at(dys + kc * 8192, role.p, 2 * role.seg)) = d[0];
        *reinterpret_cast<bf16x8d *>(dcn_tile_at(dys + kc * 8192, role.p, 2 * role.seg + 1)) = d[1];
    }
    __syncthreads();

    for (int s = 0; s < taps * chunks; ++s) {
        const int tap = s / chunks, chunk = s - tap * chunks;
        const int c0 = chunk * 64 + role.seg * 16;
        // the gather does not depend on the MFMA result: issue it first
        const DcnSample smp = dcn_tap_sample(off, role, g, tap, c0 / cg);
        bf16x8d v[4][2];
        dcn_gather(x, smp, role, g, c0, v);

        f32x4d acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f32x4d{0.f, 0.f, 0.f, 0.f};
        const bf16x8d *bsrc = reinterpret_cast<const bf16x8d *>(wpack_t) + (((int64_t)s * 4 + wid) * ksl) * 64 + lane;
        for (int ks = 0; ks < ksl; ++ks) {
            const bf16x8d b = bsrc[ks * 64];
            const char *tile = dys + (ks >> 1) * 8192;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bf16x8d a = *reinterpret_cast<const bf16x8d *>(dcn_tile_at(const_cast<char *>(tile), 16 * i + r, 4 * (ks & 1) + q));
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) dcol[(16 * i + 4 * q + e) * DCN_DCOL_LD + wid * 16 + r] = acc[i][e];
        __syncthreads();

        float dc[16];
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
            const f32x4d t = *reinterpret_cast<const f32x4d *>(&dcol[role.p * DCN_DCOL_LD + role.seg * 16 + e4 * 4]);
            dc[e4 * 4] = t[0]; dc[e4 * 4 + 1] = t[1]; dc[e4 * 4 + 2] = t[2]; dc[e4 * 4 + 3] = t[3];
        }
        // d(sample)/dh = hw (v2 - v0) + lw (v3 - v1),  d(sample)/dw = hh (v1 - v0) + lh (v3 - v2)   (masked corners hold zeros;
        // floor as in the forward: the right-hand derivative at integer positions - get_coordinate_weight)
        const float hh = 1.f - smp.lh, hw = 1.f - smp.lw;
        float gh = 0.f, gw = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float v0 = (float)v[0][e >> 3][e & 7], v1 = (float)v[1][e >> 3][e & 7], v2 = (float)v[2][e >> 3][e & 7], v3 = (float)v[3][e >> 3][e & 7];
            gh += dc[e] * (hw * (v2 - v0) + smp.lw * (v3 - v1));
            gw += dc[e] * (hh * (v1 - v0) + smp.lh * (v3 - v2));
        }
        if (lpg >= 2) { gh += __shfl_xor(gh, 1); gw += __shfl_xor(gw, 1); }
        if (lpg >= 4) { gh += __shfl_xor(gh, 2); gw += __shfl_xor(gw, 2); }
        if (role.live && (c0 % cg) == 0) {   // the first segment of the group owns (pixel, group, tap)
            OT *o = doff + role.m * (int64_t)(g.dg * 2 * taps) + (c0 / cg) * 2 * taps + 2 * tap;
            dcn_st(o, gh);
            dcn_st(o + 1, gw);
        }
        if (role.live) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (smp.ok[k] && smp.w[k] != 0.f) {
                    float *dst = dx32 + ((int64_t)role.img * g.H * g.W + smp.pix[k]) * g.cin + c0;
#pragma unroll
                    for (int e = 0; e < 16; ++e) unsafeAtomicAdd(dst + e, smp.w[k] * dc[e]);
                }
            }
        }
        __syncthreads();   // dcol is rewritten by the next step
    }
}

__global__ __launch_bounds__(256) void dcn_f32_to_bf16_kernel(const float *__restrict__ src, int64_t n8, __bf16 *__restrict__ dst) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        const f32x4d a = reinterpret_cast<const f32x4d *>(src)[2 * i], b = reinterpret_cast<const f32x4d *>(src)[2 * i + 1];
        bf16x8d o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = (__bf16)a[e];
            o[4 + e] = (__bf16)b[e];
        }
        reinterpret_cast<bf16x8d *>(dst)[i] = o;
    }
}

// ---- weight backward -----------------------------------------------------------------------------------------------------------------
constexpr int DCN_T_LD = 72;   // bf16 row pitch of the transposed tiles: 144 bytes, 16-byte aligned rows

// grid (P pixel ranges, chunks * cout / 64, taps); partial [P][tap][cin][cout]
template <typename OT>
__global__ __launch_bounds__(256) void dcn_wgrad_kernel(const __bf16 *__restrict__ x, const OT *__restrict__ off, const __bf16 *__restrict__ dy,
                                                        const __bf16 *__restrict__ ysaved, DcnGeo g, float *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) __bf16 colT[64 * DCN_T_LD];   // [cin of the chunk][pixel]
    __shared__ __attribute__((aligned(16))) __bf16 dyT[64 * DCN_T_LD];    // [cout of the block][pixel]
    const int64_t m_total = (int64_t)g.n_img * g.Ho * g.Wo;
    const int64_t n_tiles = (m_total + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int chunks = g.cin / 64, taps = g.kh * g.kw, cg = g.cin / g.dg;
    const int chunk = blockIdx.y % chunks, blk_n = blockIdx.y / chunks, tap = blockIdx.z;

    f32x4d acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4d{0.f, 0.f, 0.f, 0.f};

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const DcnRole role = dcn_role(tile * 64, m_total, g);
        const int c0 = chunk * 64 + role.seg * 16;
        const DcnSample smp = dcn_tap_sample(off, role, g, tap, c0 / cg);
        bf16x8d v[4][2], o[2], d[2];
        dcn_gather(x, smp, role, g, c0, v);
        dcn_load_dy(dy, ysaved, role, g.cout, blk_n * 64 + role.seg * 16, d);
        dcn_blend(smp, v, o);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            colT[(role.seg * 16 + e) * DCN_T_LD + role.p] = o[e >> 3][e & 7];
            dyT[(role.seg * 16 + e) * DCN_T_LD + role.p] = d[e >> 3][e & 7];
        }
        __syncthreads();
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const bf16x8d a = *reinterpret_cast<const bf16x8d *>(&colT[(16 * wid + r) * DCN_T_LD + hf * 32 + q * 8]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bf16x8d b = *reinterpret_cast<const bf16x8d *>(&dyT[(16 * j + r) * DCN_T_LD + hf * 32 + q * 8]);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // C layout: cin chunk*64 + 16 wid + 4 q + reg, cout blk_n*64 + 16 j + r
    float *dst = partial + ((int64_t)blockIdx.x * taps + tap) * g.cin * g.cout;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[(int64_t)(chunk * 64 + 16 * wid + 4 * q + e) * g.cout + blk_n * 64 + 16 * j + r] = acc[j][e];
}

// dweight[co][c][tap] = sum over the P partials in index order (same fold pattern as conv3x3_wgrad_reduce: fixed order, no atomics)
__global__ __launch_bounds__(256) void dcn_wgrad_reduce_kernel(const float *__restrict__ partial, int P, int taps, int cin, int cout,
                                                               float *__restrict__ dw) {
    const int64_t size = (int64_t)taps * cin * cout;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= size) return;
    float s = 0.f;
    for (int k = 0; k < P; ++k) s += partial[(int64_t)k * size + i];
    const int co = (int)(i % cout);
    const int64_t t = i / cout;
    const int c = (int)(t % cin), tap = (int)(t / cin);
    dw[((int64_t)co * cin + c) * taps + tap] = s;
}

static int dcn_wgrad_ranges(int64_t m_total, int cin, int cout, int taps) {
    const int64_t n_tiles = ceil_div(m_total, 64);
    int64_t p = (int64_t)2 * dcn_cus() / ((int64_t)taps * (cin / 64) * (cout / 64));   // two resident workgroups per CU
    if (p > n_tiles) p = n_tiles;
    if (p < 1) p = 1;
    return (int)p;
}

static int dcn_geo(DcnGeo &g, int n_img, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int dil, int dg, const char *who) {
    S2D_CHECK_ARG(dcn_supported(cin, cout, kh, kw, stride, pad, dil, 1, dg), "%s: unsupported shape cin=%d cout=%d k=%dx%d stride=%d pad=%d dil=%d dg=%d",
                  who, cin, cout, kh, kw, stride, pad, dil, dg);
    S2D_CHECK_ARG(n_img > 0 && h > 0 && w > 0, "%s: bad extent n=%d h=%d w=%d", who, n_img, h, w);
    const int ho = (h + 2 * pad - (dil * (kh - 1) + 1)) / stride + 1, wo = (w + 2 * pad - (dil * (kw - 1) + 1)) / stride + 1;
    S2D_CHECK_ARG(h + 2 * pad >= dil * (kh - 1) + 1 && w + 2 * pad >= dil * (kw - 1) + 1, "%s: input smaller than the kernel", who);
    S2D_CHECK_ARG((int64_t)n_img * h * w < (1ll << 31) / DCN_MAX_C && (int64_t)n_img * ho * wo < (1ll << 31) / 512, "%s: map too large", who);
    g = DcnGeo{n_img, h, w, cin, cout, kh, kw, stride, pad, dil, dg, ho, wo};
    return S2D_OK;
}

}  // namespace s2d

using namespace s2d;

extern "C" int s2d_deform_conv_supported(int cin, int cout, int kh, int kw, int stride, int pad, int dil, int groups, int dg) {
    return dcn_supported(cin, cout, kh, kw, stride, pad, dil, groups, dg) ? 1 : 0;
}

extern "C" size_t s2d_deform_conv_workspace_bytes(int n_img, int h, int w, int cin, int cout, int kh, int kw) {
    (void)n_img; (void)h; (void)w; (void)cin; (void)cout; (void)kh; (void)kw;
    return 0;   // the sampled columns never leave LDS
}

extern "C" int s2d_deform_conv_pack_weights_bf16(const float *weight, int cin, int cout, int kh, int kw, void *packed_fwd, void *packed_bwd,
                                                 s2d_stream_t stream) {
    S2D_CHECK_ARG(dcn_kernel_family(cin, cout, kh, kw, 1, 0, 1, 1, cin / 16), "deform_conv_pack_weights: unsupported shape %d -> %d, %dx%d", cin, cout, kh, kw);
    S2D_CHECK_ARG(weight && packed_fwd && packed_bwd, "deform_conv_pack_weights: null pointer");
    const int64_t total = (int64_t)kh * kw * cin * cout;
    hipLaunchKernelGGL(dcn_pack_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, weight, cin, cout, kh * kw,
                       (__bf16 *)packed_fwd, (__bf16 *)packed_bwd);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_deform_conv_nhwc_bf16(const void *x, const void *offset, int offset_bf16, const void *packed_fwd, int n_img, int h, int w, int cin,
                                         int cout, int kh, int kw, int stride, int pad, int dil, int dg, int relu, void *y, s2d_stream_t stream) {
    DcnGeo g;
    if (int rc = dcn_geo(g, n_img, h, w, cin, cout, kh, kw, stride, pad, dil, dg, "deform_conv")) return rc;
    S2D_CHECK_ARG(x && offset && packed_fwd && y, "deform_conv: null pointer");
    const dim3 grid(xcd_grid(ceil_div((int64_t)n_img * g.Ho * g.Wo, 64)), (unsigned)(cout / 64));
    if (offset_bf16)
        hipLaunchKernelGGL(dcn_fwd_kernel<__bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const __bf16 *)x, (const __bf16 *)offset,
                           (const __bf16 *)packed_fwd, g, relu, (__bf16 *)y);
    else
        hipLaunchKernelGGL(dcn_fwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const __bf16 *)x, (const float *)offset,
                           (const __bf16 *)packed_fwd, g, relu, (__bf16 *)y);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" size_t s2d_deform_conv_bwd_data_workspace_bytes(int n_img, int h, int w, int cin) {
    if (n_img <= 0 || h <= 0 || w <= 0 || cin <= 0) return 0;
    return align_up((size_t)n_img * h * w * cin * sizeof(float), 256);
}

extern "C" int s2d_deform_conv_bwd_data_nhwc_bf16(const void *x, const void *offset, int offset_bf16, const void *dy, const void *y_saved,
                                                  const void *packed_bwd, int n_img, int h, int w, int cin, int cout, int kh, int kw, int stride,
                                                  int pad, int dil, int dg, void *dx, void *d_offset, void *ws, size_t ws_bytes,
                                                  s2d_stream_t stream) {
    DcnGeo g;
    if (int rc = dcn_geo(g, n_img, h, w, cin, cout, kh, kw, stride, pad, dil, dg, "deform_conv_bwd_data")) return rc;
    S2D_CHECK_ARG(x && offset && dy && packed_bwd && dx && d_offset, "deform_conv_bwd_data: null pointer");
    const size_t need = s2d_deform_conv_bwd_data_workspace_bytes(n_img, h, w, cin);
    S2D_CHECK_ARG(ws && ws_bytes >= need, "deform_conv_bwd_data: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_in = (int64_t)n_img * h * w * cin;
    if (int rc = zero_async(ws, (size_t)n_in * sizeof(float), st)) return rc;
    const dim3 grid(xcd_grid(ceil_div((int64_t)n_img * g.Ho * g.Wo, 64)));
    const unsigned dys_bytes = (unsigned)(cout / 64) * 8192u;
    if (offset_bf16)
        hipLaunchKernelGGL(dcn_bwd_data_kernel<__bf16>, grid, dim3(256), dys_bytes, st, (const __bf16 *)x, (const __bf16 *)offset, (const __bf16 *)dy,
                           (const __bf16 *)y_saved, (const __bf16 *)packed_bwd, g, (float *)ws, (__bf16 *)d_offset);
    else
        hipLaunchKernelGGL(dcn_bwd_data_kernel<float>, grid, dim3(256), dys_bytes, st, (const __bf16 *)x, (const float *)offset, (const __bf16 *)dy,
                           (const __bf16 *)y_saved, (const __bf16 *)packed_bwd, g, (float *)ws, (float *)d_offset);
    S2D_LAUNCH_CHECK();
    const int64_t n8 = n_in / 8;   // cin is a multiple of 64
    hipLaunchKernelGGL(dcn_f32_to_bf16_kernel, dim3((unsigned)std::min<int64_t>(4096, ceil_div(n8, 256))), dim3(256), 0, st, (const float *)ws, n8,
                       (__bf16 *)dx);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" size_t s2d_deform_conv_wgrad_workspace_bytes(int n_img, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int dil) {
    if (!dcn_kernel_family(cin, cout, kh, kw, stride, pad, dil, 1, cin / 16) || n_img <= 0 || h <= 0 || w <= 0) return 0;
    const int ho = (h + 2 * pad - (dil * (kh - 1) + 1)) / stride + 1, wo = (w + 2 * pad - (dil * (kw - 1) + 1)) / stride + 1;
    if (ho <= 0 || wo <= 0) return 0;
    const int P = dcn_wgrad_ranges((int64_t)n_img * ho * wo, cin, cout, kh * kw);
    return align_up((size_t)P * kh * kw * cin * cout * sizeof(float), 256);
}

extern "C" int s2d_deform_conv_wgrad_nhwc_bf16(const void *x, const void *offset, int offset_bf16, const void *dy, const void *y_saved, int n_img,
                                               int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int dil, int dg,
                                               float *dweight, void *ws, size_t ws_bytes, s2d_stream_t stream) {
    DcnGeo g;
    if (int rc = dcn_geo(g, n_img, h, w, cin, cout, kh, kw, stride, pad, dil, dg, "deform_conv_wgrad")) return rc;
    S2D_CHECK_ARG(x && offset && dy && dweight, "deform_conv_wgrad: null pointer");
    const size_t need = s2d_deform_conv_wgrad_workspace_bytes(n_img, h, w, cin, cout, kh, kw, stride, pad, dil);
    S2D_CHECK_ARG(ws && ws_bytes >= need, "deform_conv_wgrad: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int taps = kh * kw;
    const int P = dcn_wgrad_ranges((int64_t)n_img * g.Ho * g.Wo, cin, cout, taps);
    const dim3 grid((unsigned)P, (unsigned)((cin / 64) * (cout / 64)), (unsigned)taps);
    if (offset_bf16)
        hipLaunchKernelGGL(dcn_wgrad_kernel<__bf16>, grid, dim3(256), 0, st, (const __bf16 *)x, (const __bf16 *)offset, (const __bf16 *)dy,
                           (const __bf16 *)y_saved, g, (float *)ws);
    else
        hipLaunchKernelGGL(dcn_wgrad_kernel<float>, grid, dim3(256), 0, st, (const __bf16 *)x, (const float *)offset, (const __bf16 *)dy,
                           (const __bf16 *)y_saved, g, (float *)ws);
    S2D_LAUNCH_CHECK();
    const int64_t size = (int64_t)taps * cin * cout;
    hipLaunchKernelGGL(dcn_wgrad_reduce_kernel, dim3((unsigned)ceil_div(size, 256)), dim3(256), 0, st, (const float *)ws, P, taps, cin, cout, dweight);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
