// Frame preparation of the S2D data step (det3d/datasets/pipelines/preprocess.py:81-117,178-201,257-260): the strict inside test of
// box_np_ops.points_in_rbbox, the composition of the dense and the reconstruction cloud, the four global perturbations and the shuffle gather.
//
// Inside test (fp32, no contraction): d = p - centre, |d.x cos r - d.y sin r| < dim0 / 2, |d.x sin r + d.y cos r| < dim1 / 2, |d.z| < dim2 / 2.
// prep_stage_kernel writes every box once as (centre, half extents, cos r, sin r, cos(pi/2 + r), sin(pi/2 + r)) - the angles in double,
// rounded to fp32, which is what numpy's cos / sin of the fp32 yaw give - and every other kernel copies that table into LDS once per
// workgroup; a thread owns one point and the box loop reads LDS wave-uniformly (a broadcast, no bank conflicts).
//
// Composition = counts, a scan, one order-preserving fill; the [N][M] matrix never exists:
//   prep_count_kernel     frame waves: per (wave, box) the popcount of the inside ballot, plus the wave's points outside every box, as one
//                         row of cnt [waves][M + 1].  Stored-object threads: one stored point each - its object by binary search in the
//                         offsets, the sign of y, and whether the transformed point and its mirror image lie inside any box (4 flag bits).
//   prep_scan_kernel      workgroup c <= M: exclusive prefix of column c of cnt in place, its total to coltotal[c]; workgroup M + 1 + j: the
//                         flag counts of stored object j (points per side, rows that survive the reconstruction filter).
//   prep_segments_kernel  one workgroup: the VEHICLE side (strictly more points, a tie takes y < 0), each box's block length in both
//                         clouds, their exclusive prefixes, and the two cloud sizes - the frame's one host read.
//   prep_fill_kernel      frame waves repeat the inside loop: row = block base + the wave's column prefix + the lane's rank in the ballot,
//                         i.e. input order.  One workgroup per stored object walks its points in tiles with a running rank (kept side
//                         first, then its mirror image), rotates by pi/2 + yaw and translates.
// Counting and filling evaluate the same device function on the same operands, so they agree on every membership; all counts are integers
// and there is no floating-point atomic: two calls give the same bits.
#include "s2d_common.h"
#include "box_collision.h"
#include "scan.h"

namespace s2d {
namespace {

constexpr int PREP_THREADS = 256;
constexpr int PREP_WAVES = PREP_THREADS / 64;
constexpr int PREP_MAX_BOXES = S2D_PREP_MAX_BOXES;
constexpr int PREP_BOX_F = 10;   // staged floats per box: centre 3, half extents 3, cos, sin, object cos, object sin
constexpr int PREP_OBJ_CNT = 8;  // per stored object: pos, neg, pos in orig, pos in mirror, neg in orig, neg in mirror, all in orig, unused
// per-box state bits
constexpr int PREP_STORED = 1, PREP_VEHICLE = 2, PREP_SIGN = 4, PREP_SIDE_POS = 8;
// per stored point flag bits
constexpr int PREP_F_POS = 1, PREP_F_NEG = 2, PREP_F_IN = 4, PREP_F_IN_MIRROR = 8;

struct PrepWs {
    float *table;     // [M][PREP_BOX_F]
    int *state;       // [M]
    int *range;       // [M][2]   sanitised [lo, hi) of the object's stored rows
    int *cnt;         // [waves][M + 1]
    int *coltotal;    // [M + 1]
    int *objcnt;      // [M][PREP_OBJ_CNT]
    int *seg;         // [M][4]   dense base, reconstruction base, kept points, kept rows inside (original image)
    uint8_t *flags;   // [P]
    size_t bytes;
};

int64_t prep_frame_blocks(int64_t n) { return ceil_div(n, PREP_THREADS); }

PrepWs prep_carve(void *ws, int64_t n, int m, int64_t p) {
    Carver c(ws);
    PrepWs w;
    w.table = c.take<float>((size_t)m * PREP_BOX_F);
    w.state = c.take<int>((size_t)m);
    w.range = c.take<int>((size_t)m * 2);
    w.cnt = c.take<int>((size_t)(prep_frame_blocks(n) * PREP_WAVES) * (size_t)(m + 1));
    w.coltotal = c.take<int>((size_t)m + 1);
    w.objcnt = c.take<int>((size_t)m * PREP_OBJ_CNT);
    w.seg = c.take<int>((size_t)m * 4);
    w.flags = c.take<uint8_t>((size_t)p);
    w.bytes = c.total();
    return w;
}

__device__ __forceinline__ bool prep_inside(const float *b, float x, float y, float z) {
    const float dx = x - b[0], dy = y - b[1], dz = z - b[2];
    const float lx = dx * b[6] - dy * b[7], ly = dx * b[7] + dy * b[6];
    return fabsf(lx) < b[3] && fabsf(ly) < b[4] && fabsf(dz) < b[5];
}

__device__ __forceinline__ void prep_load_table(float *lds, const float *table, int m) {
    for (int i = threadIdx.x; i < m * PREP_BOX_F; i += blockDim.x) lds[i] = table[i];
}

__device__ __forceinline__ int prep_lane_rank(unsigned long long mask) {
    const int lane = threadIdx.x & 63;
    return __popcll(mask & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(PREP_THREADS) void prep_stage_kernel(const float *boxes, int m, int box_dim, const int8_t *kinds,
                                                                   const int32_t *offsets, int p, float *table, int *state, int *range) {
    const int j = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (j >= m) return;
    const float *b = boxes + (size_t)j * box_dim;
    const double r = (double)b[box_dim - 1];
    float *t = table + (size_t)j * PREP_BOX_F;
    t[0] = b[0], t[1] = b[1], t[2] = b[2];
    t[3] = b[3] * 0.5f, t[4] = b[4] * 0.5f, t[5] = b[5] * 0.5f;
    t[6] = (float)cos(r), t[7] = (float)sin(r);
    t[8] = (float)cos(1.5707963267948966 + r), t[9] = (float)sin(1.5707963267948966 + r);
    if (!state) return;
    int lo = 0, hi = 0;
    if (offsets) {
        lo = min(max(offsets[j], 0), p);
        hi = min(max(offsets[j + 1], lo), p);
    }
    const int kind = kinds ? kinds[j] : 0;
    int s = kind == 1 ? PREP_VEHICLE : kind == 2 ? PREP_SIGN : 0;
    if (kind != 2 && hi > lo) s |= PREP_STORED;
    state[j] = s;
    range[2 * j] = lo, range[2 * j + 1] = hi;
}

// mask [N][M] (bool bytes) of the public inside test; not part of the composition
__global__ __launch_bounds__(PREP_THREADS) void prep_mask_kernel(const float *points, int64_t n, int ncols, const float *table, int m, uint8_t *mask) {
    __shared__ float box[PREP_MAX_BOXES * PREP_BOX_F];
    prep_load_table(box, table, m);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x;
    if (i >= n) return;
    const float x = points[i * ncols], y = points[i * ncols + 1], z = points[i * ncols + 2];
    uint8_t *row = mask + i * m;
    for (int j = 0; j < m; ++j) row[j] = prep_inside(box + j * PREP_BOX_F, x, y, z) ? 1 : 0;
}

// largest j with lo[j] <= p (packed offsets: the one object whose range holds p)
__device__ __forceinline__ int prep_object_of(const int *lo, int m, int p) {
    int a = 0, b = m;   // first j in [a, b) with lo[j] > p
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (lo[mid] <= p) a = mid + 1;
        else b = mid;
    }
    return a - 1;
}

__global__ __launch_bounds__(PREP_THREADS) void prep_count_kernel(const float *points, int64_t n, int ncols, const float *table, int m,
                                                                   const float *obj_points, int p, const int *state, const int *range,
                                                                   int frame_blocks, int *cnt, uint8_t *flags) {
    __shared__ float box[PREP_MAX_BOXES * PREP_BOX_F];
    __shared__ int wcnt[PREP_WAVES][PREP_MAX_BOXES + 1];
    prep_load_table(box, table, m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x < frame_blocks) {
        __syncthreads();
        const int64_t i = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x;
        const bool valid = i < n;
        float x = 0.f, y = 0.f, z = 0.f;
        if (valid) x = points[i * ncols], y = points[i * ncols + 1], z = points[i * ncols + 2];
        bool any = false;
        for (int j = 0; j < m; ++j) {
            const bool in = valid && prep_inside(box + j * PREP_BOX_F, x, y, z);
            any |= in;
            const unsigned long long mask = __ballot(in);
            if (lane == 0) wcnt[wave][j] = __popcll(mask);
        }
        const unsigned long long out = __ballot(valid && !any);
        if (lane == 0) wcnt[wave][m] = __popcll(out);
        __syncthreads();
        int *row = cnt + ((size_t)blockIdx.x * PREP_WAVES + wave) * (size_t)(m + 1);
        for (int j = lane; j <= m; j += 64) row[j] = wcnt[wave][j];
        return;
    }
    // one stored point per thread
    int *lo = &wcnt[0][0];
    for (int j = threadIdx.x; j < m; j += PREP_THREADS) lo[j] = range[2 * j];
    __syncthreads();
    const int q = ((int)blockIdx.x - frame_blocks) * PREP_THREADS + threadIdx.x;
    if (q >= p) return;
    const int j = prep_object_of(lo, m, q);
    int f = 0;
    if (j >= 0 && (state[j] & PREP_STORED) && q < range[2 * j + 1]) {
        const float *b = box + j * PREP_BOX_F;
        const float x = obj_points[(size_t)q * ncols], y = obj_points[(size_t)q * ncols + 1], z = obj_points[(size_t)q * ncols + 2];
        const float c = b[8], s = b[9];
        const float ox = (x * c + y * s) + b[0], oy = (x * -s + y * c) + b[1], oz = z + b[2];
        const float my = -y;
        const float mx = (x * c + my * s) + b[0], myy = (x * -s + my * c) + b[1];
        if (y > 0.f) f |= PREP_F_POS;
        if (y < 0.f) f |= PREP_F_NEG;
        bool in = false, in_m = false;
        for (int k = 0; k < m; ++k) {
            in |= prep_inside(box + k * PREP_BOX_F, ox, oy, oz);
            in_m |= prep_inside(box + k * PREP_BOX_F, mx, myy, oz);
        }
        if (in) f |= PREP_F_IN;
        if (in_m) f |= PREP_F_IN_MIRROR;
    }
    flags[q] = (uint8_t)f;
}

__global__ __launch_bounds__(PREP_THREADS) void prep_scan_kernel(int *cnt, int rows, int m, int *coltotal, const uint8_t *flags, const int *state,
                                                                  const int *range, int *objcnt) {
    __shared__ int lds[PREP_OBJ_CNT];
    if ((int)blockIdx.x <= m) {
        const int c = blockIdx.x;
        const int chunk = (rows + PREP_THREADS - 1) / PREP_THREADS;
        const int r0 = min(rows, (int)threadIdx.x * chunk), r1 = min(rows, r0 + chunk);
        int s = 0;
        for (int r = r0; r < r1; ++r) s += cnt[(size_t)r * (m + 1) + c];
        int total;
        int run = block_exclusive_scan(s, &total, lds);
        for (int r = r0; r < r1; ++r) {
            int *e = cnt + (size_t)r * (m + 1) + c;
            const int v = *e;
            *e = run;
            run += v;
        }
        if (threadIdx.x == 0) coltotal[c] = total;
        return;
    }
    const int j = (int)blockIdx.x - (m + 1);
    if (threadIdx.x < PREP_OBJ_CNT) lds[threadIdx.x] = 0;
    __syncthreads();
    int acc[PREP_OBJ_CNT - 1] = {0, 0, 0, 0, 0, 0, 0};
    if (state[j] & PREP_STORED) {
        for (int q = range[2 * j] + threadIdx.x; q < range[2 * j + 1]; q += PREP_THREADS) {
            const int f = flags[q];
            const bool pos = f & PREP_F_POS, neg = f & PREP_F_NEG, in = f & PREP_F_IN, in_m = f & PREP_F_IN_MIRROR;
            acc[0] += pos, acc[1] += neg;
            acc[2] += pos && in, acc[3] += pos && in_m;
            acc[4] += neg && in, acc[5] += neg && in_m;
            acc[6] += in;
        }
    }
#pragma unroll
    for (int k = 0; k < PREP_OBJ_CNT - 1; ++k)
        if (acc[k]) atomicAdd(&lds[k], acc[k]);   // integer sums in LDS: the order does not matter
    __syncthreads();
    if (threadIdx.x < PREP_OBJ_CNT) objcnt[j * PREP_OBJ_CNT + threadIdx.x] = lds[threadIdx.x];
}

__global__ __launch_bounds__(PREP_THREADS) void prep_segments_kernel(int m, int *state, const int *range, const int *coltotal, const int *objcnt,
                                                                      int *seg, int32_t *totals) {
    __shared__ int lds[4];
    int dense_run = coltotal[m], recon_run = 0, not_sign = 0;   // the points outside every box come first
    for (int base = 0; base < m; base += PREP_THREADS) {
        const int j = base + threadIdx.x;
        int dense_len = 0, recon_len = 0, kept = 0, kept_in = 0, s = 0;
        if (j < m) {
            s = state[j] & ~PREP_SIDE_POS;
            const int *oc = objcnt + j * PREP_OBJ_CNT;
            if (s & PREP_STORED) {
                if (s & PREP_VEHICLE) {
                    const bool pos = oc[0] > oc[1];
                    if (pos) s |= PREP_SIDE_POS;
                    kept = pos ? oc[0] : oc[1];
                    kept_in = pos ? oc[2] : oc[4];
                    dense_len = 2 * kept;
                    recon_len = kept_in + (pos ? oc[3] : oc[5]);
                } else {
                    kept = range[2 * j + 1] - range[2 * j];
                    kept_in = oc[6];
                    dense_len = kept;
                    recon_len = kept_in;
                }
            } else {
                dense_len = coltotal[j];
                recon_len = (s & PREP_SIGN) ? 0 : dense_len;
            }
        }
        int dense_tot, recon_tot, not_sign_tot;
        const int dense_ex = block_exclusive_scan(dense_len, &dense_tot, lds);
        const int recon_ex = block_exclusive_scan(recon_len, &recon_tot, lds);
        block_exclusive_scan((int)(j < m && !(s & PREP_SIGN)), &not_sign_tot, lds);
        if (j < m) {
            state[j] = s;
            seg[4 * j] = dense_run + dense_ex, seg[4 * j + 1] = recon_run + recon_ex, seg[4 * j + 2] = kept, seg[4 * j + 3] = kept_in;
        }
        dense_run += dense_tot, recon_run += recon_tot, not_sign += not_sign_tot;
    }
    if (threadIdx.x == 0) totals[0] = dense_run, totals[1] = recon_run, totals[2] = not_sign;
}

__device__ __forceinline__ void prep_copy_row(float *dst, const float *src, int ncols) {
    for (int c = 0; c < ncols; ++c) dst[c] = src[c];
}

__global__ __launch_bounds__(PREP_THREADS) void prep_fill_kernel(const float *points, int64_t n, int ncols, const float *table, int m,
                                                                  const float *obj_points, const int *state, const int *range, const int *cnt,
                                                                  const int *seg, const uint8_t *flags, int frame_blocks, float *dense,
                                                                  int dense_rows, float *recon, int recon_rows) {
    __shared__ float box[PREP_MAX_BOXES * PREP_BOX_F];
    __shared__ int lds[4];
    const int wave = threadIdx.x >> 6;
    if ((int)blockIdx.x < frame_blocks) {
        prep_load_table(box, table, m);
        __syncthreads();
        const int64_t i = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x;
        const bool valid = i < n;
        float x = 0.f, y = 0.f, z = 0.f;
        if (valid) x = points[i * ncols], y = points[i * ncols + 1], z = points[i * ncols + 2];
        const int *prefix = cnt + ((size_t)blockIdx.x * PREP_WAVES + wave) * (size_t)(m + 1);
        bool any = false;
        for (int j = 0; j < m; ++j) {
            const bool in = valid && prep_inside(box + j * PREP_BOX_F, x, y, z);
            any |= in;
            const unsigned long long mask = __ballot(in);
            if (mask == 0ull) continue;   // wave-uniform
            const int s = state[j];
            if (s & PREP_STORED) continue;
            if (in) {
                const int rank = prefix[j] + prep_lane_rank(mask);
                const int d = seg[4 * j] + rank;
                if (d < dense_rows) prep_copy_row(dense + (size_t)d * ncols, points + i * ncols, ncols);
                if (!(s & PREP_SIGN)) {
                    const int r = seg[4 * j + 1] + rank;
                    if (r < recon_rows) prep_copy_row(recon + (size_t)r * ncols, points + i * ncols, ncols);
                }
            }
        }
        const bool out = valid && !any;
        const unsigned long long mask = __ballot(out);
        if (out) {
            const int d = prefix[m] + prep_lane_rank(mask);
            if (d < dense_rows) prep_copy_row(dense + (size_t)d * ncols, points + i * ncols, ncols);
        }
        return;
    }
    // one stored object per workgroup, its rows in tiles with a running rank
    const int j = (int)blockIdx.x - frame_blocks;
    const int s = state[j];
    if (!(s & PREP_STORED)) return;
    const float *b = table + (size_t)j * PREP_BOX_F;
    const float bx = b[0], by = b[1], bz = b[2], c = b[8], sn = b[9];
    const bool vehicle = s & PREP_VEHICLE;
    const int side = (s & PREP_SIDE_POS) ? PREP_F_POS : PREP_F_NEG;
    const int lo = range[2 * j], hi = range[2 * j + 1];
    const int dense0 = seg[4 * j], recon0 = seg[4 * j + 1], kept_all = seg[4 * j + 2], kept_in_all = seg[4 * j + 3];
    int run_keep = 0, run_in = 0, run_in_m = 0;
    for (int base = lo; base < hi; base += PREP_THREADS) {
        const int q = base + threadIdx.x;
        int f = 0;
        bool keep = false;
        if (q < hi) {
            f = flags[q];
            keep = !vehicle || (f & side);
        }
        const bool in = keep && (f & PREP_F_IN), in_m = keep && vehicle && (f & PREP_F_IN_MIRROR);
        // three counts of at most 256 each in one scan: 10 bits apiece
        const int packed = (int)keep | ((int)in << 10) | ((int)in_m << 20);
        int total;
        const int ex = block_exclusive_scan(packed, &total, lds);
        if (keep) {
            const float *src = obj_points + (size_t)q * ncols;
            const float x = src[0], y = src[1], z = src[2];
            const int k = run_keep + (ex & 1023);
            const float ox = (x * c + y * sn) + bx, oy = (x * -sn + y * c) + by, oz = z + bz;
            const int d = dense0 + k;
            if (d < dense_rows) {
                float *dst = dense + (size_t)d * ncols;
                dst[0] = ox, dst[1] = oy, dst[2] = oz;
                for (int e = 3; e < ncols; ++e) dst[e] = src[e];
            }
            if (in) {
                const int r = recon0 + run_in + ((ex >> 10) & 1023);
                if (r < recon_rows) {
                    float *dst = recon + (size_t)r * ncols;
                    dst[0] = ox, dst[1] = oy, dst[2] = oz;
                    for (int e = 3; e < ncols; ++e) dst[e] = src[e];
                }
            }
            if (vehicle) {
                const float my = -y;
                const float mx = (x * c + my * sn) + bx, myy = (x * -sn + my * c) + by;
                const int dm = dense0 + kept_all + k;
                if (dm < dense_rows) {
                    float *dst = dense + (size_t)dm * ncols;
                    dst[0] = mx, dst[1] = myy, dst[2] = oz;
                    for (int e = 3; e < ncols; ++e) dst[e] = src[e];
                }
                if (in_m) {
                    const int r = recon0 + kept_in_all + run_in_m + ((ex >> 20) & 1023);
                    if (r < recon_rows) {
                        float *dst = recon + (size_t)r * ncols;
                        dst[0] = mx, dst[1] = myy, dst[2] = oz;
                        for (int e = 3; e < ncols; ++e) dst[e] = src[e];
                    }
                }
            }
        }
        run_keep += total & 1023, run_in += (total >> 10) & 1023, run_in_m += (total >> 20) & 1023;
    }
}

struct NoiseArgs {
    float *cloud[3];
    int64_t rows[3];
    int ncols, flip_x, flip_y, translate;
    float rot_cos, rot_sin, scale;
    double t[3];
};

// preprocess.py:859-908,790-813,1032-1056 on columns 0-2: y flip, x flip, rotation about z, scale, translation (added in double, as numpy
// adds its float64 draw to the fp32 column)
__global__ __launch_bounds__(PREP_THREADS) void prep_noise_kernel(NoiseArgs a) {
    int64_t i = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x;
    float *p = nullptr;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!p && i < a.rows[k]) p = a.cloud[k] + i * a.ncols;
        if (!p) i -= a.rows[k];
    }
    if (!p) return;
    float x = p[0], y = p[1], z = p[2];
    if (a.flip_x) y = -y;
    if (a.flip_y) x = -x;
    float xr = x * a.rot_cos + y * a.rot_sin, yr = x * -a.rot_sin + y * a.rot_cos;
    xr *= a.scale, yr *= a.scale, z *= a.scale;
    if (a.translate) {
        xr = (float)((double)xr + a.t[0]), yr = (float)((double)yr + a.t[1]), z = (float)((double)z + a.t[2]);
    }
    p[0] = xr, p[1] = yr, p[2] = z;
}

__global__ __launch_bounds__(PREP_THREADS) void prep_gather_kernel(const float *src, int64_t n, int ncols, const int64_t *perm, float *dst) {
    const int64_t e = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x;
    if (e >= n * ncols) return;
    const int64_t row = e / ncols;
    const int64_t from = perm[row];
    if (from < 0 || from >= n) return;   // not a permutation: the row stays unwritten rather than read out of bounds
    dst[e] = src[from * ncols + (e - row * ncols)];
}

int prep_check_sizes(const char *what, int64_t n, int ncols, int m, int box_dim, int64_t p) {
    S2D_CHECK_ARG(n >= 0 && n <= S2D_PREP_MAX_POINTS, "%s: n_points %lld (0..%d)", what, (long long)n, S2D_PREP_MAX_POINTS);
    S2D_CHECK_ARG(p >= 0 && p <= S2D_PREP_MAX_POINTS, "%s: %lld stored object points (0..%d)", what, (long long)p, S2D_PREP_MAX_POINTS);
    S2D_CHECK_ARG(ncols >= 3 && ncols <= 16, "%s: %d point columns (3..16)", what, ncols);
    S2D_CHECK_ARG(m >= 0 && m <= PREP_MAX_BOXES, "%s: %d boxes (0..%d supported)", what, m, PREP_MAX_BOXES);
    S2D_CHECK_ARG(m == 0 || box_dim >= 7, "%s: box_dim %d (>= 7: centre, size, ..., yaw last)", what, box_dim);
    return S2D_OK;
}

int prep_stage(const float *boxes, int m, int box_dim, const int8_t *kinds, const int32_t *offsets, int p, const PrepWs &w, bool with_state,
               hipStream_t st) {
    if (m == 0) return S2D_OK;
    hipLaunchKernelGGL(prep_stage_kernel, dim3((unsigned)ceil_div(m, PREP_THREADS)), dim3(PREP_THREADS), 0, st, boxes, m, box_dim, kinds, offsets, p,
                       w.table, with_state ? w.state : nullptr, w.range);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

// ---- GT-database sampler (det3d/core/sampler/sample_ops.py:134-359) -----------------------------------------------------------------------------
// gt_select_kernel    ONE workgroup for all groups of a frame: corners and stand-up boxes of the M avoid boxes and the S candidates in LDS, the
//                     S x (M + S) bit matrix of box_collision_test in LDS (a wave owns a row word: one pair per lane, the ballot is the word),
//                     then one wave walks groups and candidates in order against the alive mask (lane w holds word w), then the accepted
//                     blocks' exclusive row offsets.
// gt_count_kernel     one workgroup per accepted candidate: the rows of its completed cloud per side of y and strictly inside its OWN box
//                     (original and mirror image), the VEHICLE side, the length of its reconstruction block.
// gt_segments_kernel  one workgroup: exclusive prefix of the reconstruction block lengths, their total to the header.
// gt_paste_kernel     one workgroup per accepted candidate: its sweep rows plus the box centre to the front of the new sweep and dense cloud,
//                     its reconstruction block (order-preserving, kept side first, then the mirror image) to the front of the new
//                     reconstruction cloud.
constexpr int GT_MAX_CAND = S2D_PREP_MAX_CANDIDATES;
constexpr int GT_MAX_GROUPS = S2D_PREP_MAX_GROUPS;
constexpr int GT_WORDS = PREP_MAX_BOXES / 64;
constexpr int GT_META = 5;   // per candidate: sweep rows lo, hi; completed cloud rows lo, hi; kind
constexpr int GT_SEG = 6;    // per candidate: sweep base, reconstruction base, reconstruction length, kept rows, kept rows inside, side y > 0

struct GtGroups {
    int end[GT_MAX_GROUPS];   // exclusive end of each group's candidates
    int n;
};

struct GtWs {
    float *table;   // [S][PREP_BOX_F]
    int *range;     // [S][4]  sanitised meta ranges
    int *seg;       // [S][GT_SEG]
    size_t bytes;
};

GtWs gt_carve(void *ws, int s) {
    Carver c(ws);
    GtWs w;
    w.table = c.take<float>((size_t)s * PREP_BOX_F);
    w.range = c.take<int>((size_t)s * 4);
    w.seg = c.take<int>((size_t)s * GT_SEG);
    w.bytes = c.total();
    return w;
}

__global__ __launch_bounds__(PREP_THREADS) void prep_collision_kernel(const float *corners, int n, const float *qcorners, int k, uint8_t *out) {
    const int64_t e = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x;
    if (e >= (int64_t)n * k) return;
    const int i = (int)(e / k), j = (int)(e - (int64_t)i * k);
    float b[8], q[8], bs[4], qs[4];
#pragma unroll
    for (int t = 0; t < 8; ++t) b[t] = corners[(size_t)i * 8 + t], q[t] = qcorners[(size_t)j * 8 + t];
    standup_of(b, bs);
    standup_of(q, qs);
    out[e] = box_pair_collides(b, bs, q, qs) ? 1 : 0;
}

__global__ __launch_bounds__(PREP_THREADS) void gt_select_kernel(const float *boxes, int m, int s, int box_dim, GtGroups groups, const int32_t *meta,
                                                                  int64_t src_rows, int64_t cc_rows, float *table, int *range, int *seg,
                                                                  int32_t *header) {
    __shared__ float corner[PREP_MAX_BOXES * 8];
    __shared__ float standup[PREP_MAX_BOXES * 4];
    __shared__ unsigned long long bits[GT_MAX_CAND * GT_WORDS];
    __shared__ int accept[GT_MAX_CAND];
    __shared__ int lds[4];
    const int total = m + s, words = (total + 63) >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = threadIdx.x; j < total; j += PREP_THREADS) {
        const float *b = boxes + (size_t)j * box_dim;
        bev_corners_of(b, box_dim, corner + 8 * j, standup + 4 * j);
        if (j >= m) {   // the candidate's staged box (inside test, rotation by pi/2 + yaw) and its sanitised row ranges
            const int i = j - m;
            const double r = (double)b[box_dim - 1];
            float *t = table + (size_t)i * PREP_BOX_F;
            t[0] = b[0], t[1] = b[1], t[2] = b[2];
            t[3] = b[3] * 0.5f, t[4] = b[4] * 0.5f, t[5] = b[5] * 0.5f;
            t[6] = (float)cos(r), t[7] = (float)sin(r);
            t[8] = (float)cos(1.5707963267948966 + r), t[9] = (float)sin(1.5707963267948966 + r);
            const int32_t *mt = meta + (size_t)i * GT_META;
            const int lo = (int)min((int64_t)max(mt[0], 0), src_rows), hi = (int)min((int64_t)max(mt[1], lo), src_rows);
            const int clo = (int)min((int64_t)max(mt[2], 0), cc_rows), chi = (int)min((int64_t)max(mt[3], clo), cc_rows);
            range[4 * i] = lo, range[4 * i + 1] = hi, range[4 * i + 2] = clo, range[4 * i + 3] = chi;
        }
    }
    __syncthreads();
    // bits[i][w]: row i = candidate i as `boxes`, column j = box j as `qboxes`; the diagonal is clear
    for (int item = wave; item < s * words; item += PREP_WAVES) {
        const int i = item / words, w = item - i * words;
        const int j = w * 64 + lane;
        bool hit = false;
        if (j < total && j != m + i) hit = box_pair_collides(corner + 8 * (m + i), standup + 4 * (m + i), corner + 8 * j, standup + 4 * j);
        const unsigned long long word = __ballot(hit);
        if (lane == 0) bits[i * GT_WORDS + w] = word;
    }
    __syncthreads();
    if (wave == 0) {
        // lane w < words holds word w of the alive mask: the avoid boxes always, a group's candidates from its start until rejected
        unsigned long long alive = 0ull;
        if (lane < words) {
            const int lo = lane * 64;
            if (m >= lo + 64) alive = ~0ull;
            else if (m > lo) alive = (1ull << (m - lo)) - 1ull;
        }
        int start = 0;
        for (int g = 0; g < groups.n; ++g) {
            const int end = min(max(groups.end[g], start), s);
            if (lane < words) {
                const int lo = lane * 64;
                for (int i = start; i < end; ++i) {
                    const int col = m + i - lo;
                    if (col >= 0 && col < 64) alive |= 1ull << col;
                }
            }
            for (int i = start; i < end; ++i) {
                const unsigned long long row = lane < words ? bits[i * GT_WORDS + lane] & alive : 0ull;
                const bool rejected = __ballot(row != 0ull) != 0ull;   // wave-uniform
                if (rejected) {
                    const int col = m + i - lane * 64;
                    if (col >= 0 && col < 64) alive &= ~(1ull << col);
                }
                if (lane == 0) accept[i] = rejected ? 0 : 1;
            }
            start = end;
        }
        for (int i = start + lane; i < s; i += 64) accept[i] = 0;   // candidates beyond the last group belong to none
    }
    __syncthreads();
    const int i = threadIdx.x;
    const int ok = i < s ? accept[i] : 0;
    const int rows = ok ? range[4 * i + 1] - range[4 * i] : 0;
    int rows_total;
    const int base = block_exclusive_scan(rows, &rows_total, lds);
    if (i < s) {
        seg[GT_SEG * i] = base;
        header[2 + i] = ok;
    }
    if (i == 0) header[0] = rows_total;
}

// flag bits of one completed-cloud row against the candidate's own box: the sign of y, the image and the mirror image strictly inside
__device__ __forceinline__ int gt_row_flags(const float *t, const float *row, float *out /*ox oy oz mx my*/) {
    const float x = row[0], y = row[1], z = row[2];
    const float c = t[8], s = t[9];
    out[0] = (x * c + y * s) + t[0], out[1] = (x * -s + y * c) + t[1], out[2] = z + t[2];
    const float my = -y;
    out[3] = (x * c + my * s) + t[0], out[4] = (x * -s + my * c) + t[1];
    int f = 0;
    if (y > 0.f) f |= PREP_F_POS;
    if (y < 0.f) f |= PREP_F_NEG;
    if (prep_inside(t, out[0], out[1], out[2])) f |= PREP_F_IN;
    if (prep_inside(t, out[3], out[4], out[2])) f |= PREP_F_IN_MIRROR;
    return f;
}

__global__ __launch_bounds__(PREP_THREADS) void gt_count_kernel(int s, int ncols, const int32_t *meta, const float *cc_points, const float *table,
                                                                 const int *range, int *seg, const int32_t *header) {
    __shared__ int cnt[PREP_OBJ_CNT];
    __shared__ float t[PREP_BOX_F];
    const int i = blockIdx.x;
    int *sg = seg + GT_SEG * i;
    const int lo = range[4 * i], hi = range[4 * i + 1], clo = range[4 * i + 2], chi = range[4 * i + 3];
    if (!header[2 + i] || chi <= clo) {   // rejected: nothing; no completed cloud: the reconstruction block is the sampled rows
        if (threadIdx.x == 0) sg[2] = header[2 + i] ? hi - lo : 0, sg[3] = 0, sg[4] = 0, sg[5] = 0;
        return;
    }
    if (threadIdx.x < PREP_OBJ_CNT) cnt[threadIdx.x] = 0;
    if (threadIdx.x < PREP_BOX_F) t[threadIdx.x] = table[(size_t)i * PREP_BOX_F + threadIdx.x];
    __syncthreads();
    int acc[PREP_OBJ_CNT - 1] = {0, 0, 0, 0, 0, 0, 0};
    for (int q = clo + threadIdx.x; q < chi; q += PREP_THREADS) {
        float o[5];
        const int f = gt_row_flags(t, cc_points + (size_t)q * ncols, o);
        const bool pos = f & PREP_F_POS, neg = f & PREP_F_NEG, in = f & PREP_F_IN, in_m = f & PREP_F_IN_MIRROR;
        acc[0] += pos, acc[1] += neg;
        acc[2] += pos && in, acc[3] += pos && in_m;
        acc[4] += neg && in, acc[5] += neg && in_m;
        acc[6] += in;
    }
#pragma unroll
    for (int k = 0; k < PREP_OBJ_CNT - 1; ++k)
        if (acc[k]) atomicAdd(&cnt[k], acc[k]);   // integer sums in LDS: the order does not matter
    __syncthreads();
    if (threadIdx.x == 0) {
        if (meta[(size_t)i * GT_META + 4] == 1) {   // VEHICLE: strictly more rows with y > 0 keeps that side, a tie keeps y < 0
            const bool pos = cnt[0] > cnt[1];
            sg[3] = pos ? cnt[0] : cnt[1];
            sg[4] = pos ? cnt[2] : cnt[4];
            sg[2] = sg[4] + (pos ? cnt[3] : cnt[5]);
            sg[5] = pos;
        } else {
            sg[3] = chi - clo, sg[4] = cnt[6], sg[2] = cnt[6], sg[5] = 0;
        }
    }
}

__global__ __launch_bounds__(PREP_THREADS) void gt_segments_kernel(int s, int *seg, int32_t *header) {
    __shared__ int lds[4];
    const int i = threadIdx.x;
    int total;
    const int base = block_exclusive_scan(i < s ? seg[GT_SEG * i + 2] : 0, &total, lds);
    if (i < s) seg[GT_SEG * i + 1] = base;
    if (i == 0) header[1] = total;
}

__device__ __forceinline__ void gt_put_row(float *cloud, int row, int rows, int ncols, float x, float y, float z, const float *src) {
    if (!cloud || row >= rows) return;
    float *dst = cloud + (size_t)row * ncols;
    dst[0] = x, dst[1] = y, dst[2] = z;
    for (int e = 3; e < ncols; ++e) dst[e] = src[e];
}

__global__ __launch_bounds__(PREP_THREADS) void gt_paste_kernel(int s, int ncols, const int32_t *meta, const float *src_points, const float *cc_points,
                                                                 const float *table, const int *range, const int *seg, const int32_t *header,
                                                                 float *points_out, float *dense_out, int sampled_rows, float *recon_out,
                                                                 int recon_rows) {
    __shared__ int lds[4];
    __shared__ float t[PREP_BOX_F];
    const int i = blockIdx.x;
    if (!header[2 + i]) return;
    if (threadIdx.x < PREP_BOX_F) t[threadIdx.x] = table[(size_t)i * PREP_BOX_F + threadIdx.x];
    __syncthreads();
    const int lo = range[4 * i], hi = range[4 * i + 1], clo = range[4 * i + 2], chi = range[4 * i + 3];
    const int *sg = seg + GT_SEG * i;
    const int base = sg[0], recon0 = sg[1], kept_in_all = sg[4];
    const bool own = chi <= clo;   // no completed cloud: the sampled rows are the reconstruction block too
    for (int q = lo + threadIdx.x; q < hi; q += PREP_THREADS) {
        const float *src = src_points + (size_t)q * ncols;
        const float x = src[0] + t[0], y = src[1] + t[1], z = src[2] + t[2];
        const int k = q - lo;
        gt_put_row(points_out, base + k, sampled_rows, ncols, x, y, z, src);
        gt_put_row(dense_out, base + k, sampled_rows, ncols, x, y, z, src);
        if (own) gt_put_row(recon_out, recon0 + k, recon_rows, ncols, x, y, z, src);
    }
    if (own || !recon_out) return;
    const bool vehicle = meta[(size_t)i * GT_META + 4] == 1;
    const int side = sg[5] ? PREP_F_POS : PREP_F_NEG;
    int run_in = 0, run_in_m = 0;
    for (int b = clo; b < chi; b += PREP_THREADS) {   // (every thread takes every turn: the scan has barriers)
        const int q = b + threadIdx.x;
        float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        const float *src = cc_points + (size_t)min(q, chi - 1) * ncols;
        int f = 0;
        bool keep = false;
        if (q < chi) {
            f = gt_row_flags(t, src, o);
            keep = !vehicle || (f & side);
        }
        const bool in = keep && (f & PREP_F_IN), in_m = keep && vehicle && (f & PREP_F_IN_MIRROR);
        const int packed = (int)in | ((int)in_m << 10);   // two counts of at most 256 each in one scan
        int total;
        const int ex = block_exclusive_scan(packed, &total, lds);
        if (in) gt_put_row(recon_out, recon0 + run_in + (ex & 1023), recon_rows, ncols, o[0], o[1], o[2], src);
        if (in_m) gt_put_row(recon_out, recon0 + kept_in_all + run_in_m + ((ex >> 10) & 1023), recon_rows, ncols, o[3], o[4], o[2], src);
        run_in += total & 1023, run_in_m += (total >> 10) & 1023;
    }
}

int gt_check_sizes(const char *what, int m, int s, int box_dim, int ncols, int64_t src_rows, int64_t cc_rows) {
    S2D_CHECK_ARG(m >= 0 && s >= 1 && s <= GT_MAX_CAND, "%s: %d candidates (1..%d)", what, s, GT_MAX_CAND);
    S2D_CHECK_ARG(m + s <= PREP_MAX_BOXES, "%s: %d avoid boxes + %d candidates (at most %d boxes)", what, m, s, PREP_MAX_BOXES);
    S2D_CHECK_ARG(box_dim >= 7 && box_dim <= 16, "%s: box_dim %d (7..16: centre, size, ..., yaw last)", what, box_dim);
    S2D_CHECK_ARG(ncols >= 3 && ncols <= 16, "%s: %d point columns (3..16)", what, ncols);
    S2D_CHECK_ARG(src_rows >= 0 && src_rows <= S2D_PREP_MAX_POINTS && cc_rows >= 0 && cc_rows <= S2D_PREP_MAX_POINTS,
                  "%s: store rows %lld / %lld (0..%d)", what, (long long)src_rows, (long long)cc_rows, S2D_PREP_MAX_POINTS);
    return S2D_OK;
}

}  // namespace
}  // namespace s2d

using namespace s2d;

extern "C" size_t s2d_prep_workspace_bytes(int64_t n_points, int num_boxes, int64_t obj_rows) {
    if (n_points < 0 || n_points > S2D_PREP_MAX_POINTS || obj_rows < 0 || obj_rows > S2D_PREP_MAX_POINTS || num_boxes < 0 ||
        num_boxes > PREP_MAX_BOXES)
        return 0;
    return prep_carve(nullptr, n_points, num_boxes, obj_rows).bytes + 256;
}

extern "C" int s2d_prep_points_in_rbbox(const float *points, int64_t n_points, int ncols, const float *boxes, int num_boxes, int box_dim,
                                        uint8_t *mask, int32_t *counts, void *ws, size_t ws_bytes, s2d_stream_t stream) {
    if (int rc = prep_check_sizes("prep_points_in_rbbox", n_points, ncols, num_boxes, box_dim, 0)) return rc;
    S2D_CHECK_ARG(mask || counts, "prep_points_in_rbbox: neither a mask nor counts asked for");
    if (num_boxes == 0) return S2D_OK;
    S2D_CHECK_ARG(boxes && (n_points == 0 || points), "prep_points_in_rbbox: null points or boxes");
    const PrepWs w = prep_carve(ws, n_points, num_boxes, 0);
    if (!ws || ws_bytes < w.bytes) {
        set_error("prep_points_in_rbbox: workspace %zu bytes, %zu needed", ws_bytes, w.bytes);
        return S2D_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int m = num_boxes;
    if (int rc = prep_stage(boxes, m, box_dim, nullptr, nullptr, 0, w, false, st)) return rc;
    const int fb = (int)prep_frame_blocks(n_points);
    if (mask && fb) hipLaunchKernelGGL(prep_mask_kernel, dim3(fb), dim3(PREP_THREADS), 0, st, points, n_points, ncols, w.table, m, mask);
    if (counts) {
        if (fb)
            hipLaunchKernelGGL(prep_count_kernel, dim3(fb), dim3(PREP_THREADS), 0, st, points, n_points, ncols, w.table, m, (const float *)nullptr, 0,
                               (const int *)nullptr, (const int *)nullptr, fb, w.cnt, (uint8_t *)nullptr);
        // the column totals: the first num_boxes entries of coltotal; the scan's object part is not launched
        hipLaunchKernelGGL(prep_scan_kernel, dim3(m + 1), dim3(PREP_THREADS), 0, st, w.cnt, fb * PREP_WAVES, m, w.coltotal, (const uint8_t *)nullptr,
                           (const int *)nullptr, (const int *)nullptr, (int *)nullptr);
        S2D_HIP(hipMemcpyAsync(counts, w.coltotal, sizeof(int32_t) * m, hipMemcpyDeviceToDevice, st));
    }
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_prep_compose_count(const float *points, int64_t n_points, int ncols, const float *boxes, int num_boxes, int box_dim,
                                      const int8_t *kinds, const float *obj_points, int64_t obj_rows, const int32_t *obj_offsets, void *ws,
                                      size_t ws_bytes, int32_t *totals, s2d_stream_t stream) {
    if (int rc = prep_check_sizes("prep_compose_count", n_points, ncols, num_boxes, box_dim, obj_rows)) return rc;
    S2D_CHECK_ARG(totals, "prep_compose_count: null totals");
    S2D_CHECK_ARG(n_points == 0 || points, "prep_compose_count: null points");
    S2D_CHECK_ARG(num_boxes == 0 || (boxes && kinds), "prep_compose_count: null boxes or kinds");
    S2D_CHECK_ARG(obj_rows == 0 || (obj_points && obj_offsets && num_boxes > 0), "prep_compose_count: stored rows without points, offsets or boxes");
    const PrepWs w = prep_carve(ws, n_points, num_boxes, obj_rows);
    if (!ws || ws_bytes < w.bytes) {
        set_error("prep_compose_count: workspace %zu bytes, %zu needed", ws_bytes, w.bytes);
        return S2D_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int m = num_boxes, p = (int)obj_rows;
    if (int rc = prep_stage(boxes, m, box_dim, kinds, obj_rows ? obj_offsets : nullptr, p, w, true, st)) return rc;
    const int fb = (int)prep_frame_blocks(n_points), ob = (int)ceil_div(p, PREP_THREADS);
    if (fb + ob)
        hipLaunchKernelGGL(prep_count_kernel, dim3(fb + ob), dim3(PREP_THREADS), 0, st, points, n_points, ncols, w.table, m, obj_points, p, w.state,
                           w.range, fb, w.cnt, w.flags);
    hipLaunchKernelGGL(prep_scan_kernel, dim3(2 * m + 1), dim3(PREP_THREADS), 0, st, w.cnt, fb * PREP_WAVES, m, w.coltotal, w.flags, w.state, w.range,
                       w.objcnt);
    hipLaunchKernelGGL(prep_segments_kernel, dim3(1), dim3(PREP_THREADS), 0, st, m, w.state, w.range, w.coltotal, w.objcnt, w.seg, totals);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_prep_compose_fill(const float *points, int64_t n_points, int ncols, int num_boxes, const float *obj_points, int64_t obj_rows,
                                     const void *ws, size_t ws_bytes, float *dense, int64_t dense_rows, float *recon, int64_t recon_rows,
                                     s2d_stream_t stream) {
    if (int rc = prep_check_sizes("prep_compose_fill", n_points, ncols, num_boxes, 7, obj_rows)) return rc;
    S2D_CHECK_ARG(dense_rows >= 0 && recon_rows >= 0 && dense_rows <= 3ll * S2D_PREP_MAX_POINTS && recon_rows <= 3ll * S2D_PREP_MAX_POINTS,
                  "prep_compose_fill: output rows %lld / %lld", (long long)dense_rows, (long long)recon_rows);
    S2D_CHECK_ARG(n_points == 0 || points, "prep_compose_fill: null points");
    S2D_CHECK_ARG(obj_rows == 0 || obj_points, "prep_compose_fill: null stored points");
    S2D_CHECK_ARG((dense_rows == 0 || dense) && (recon_rows == 0 || recon), "prep_compose_fill: null output");
    const PrepWs w = prep_carve(const_cast<void *>(ws), n_points, num_boxes, obj_rows);
    if (!ws || ws_bytes < w.bytes) {
        set_error("prep_compose_fill: workspace %zu bytes, %zu needed", ws_bytes, w.bytes);
        return S2D_ERR_WORKSPACE;
    }
    const int fb = (int)prep_frame_blocks(n_points), ob = obj_rows ? num_boxes : 0;
    if (fb + ob == 0) return S2D_OK;
    hipLaunchKernelGGL(prep_fill_kernel, dim3(fb + ob), dim3(PREP_THREADS), 0, (hipStream_t)stream, points, n_points, ncols, w.table, num_boxes,
                       obj_points, w.state, w.range, w.cnt, w.seg, w.flags, fb, dense, (int)dense_rows, recon, (int)recon_rows);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_prep_global_noise(float *cloud0, int64_t rows0, float *cloud1, int64_t rows1, float *cloud2, int64_t rows2, int ncols, int flip_x,
                                     int flip_y, float rot_cos, float rot_sin, float scale, int translate, double tx, double ty, double tz,
                                     s2d_stream_t stream) {
    S2D_CHECK_ARG(ncols >= 3 && ncols <= 16, "prep_global_noise: %d point columns (3..16)", ncols);
    S2D_CHECK_ARG(rows0 >= 0 && rows1 >= 0 && rows2 >= 0 && rows0 <= 3ll * S2D_PREP_MAX_POINTS && rows1 <= 3ll * S2D_PREP_MAX_POINTS &&
                      rows2 <= 3ll * S2D_PREP_MAX_POINTS,
                  "prep_global_noise: rows %lld / %lld / %lld", (long long)rows0, (long long)rows1, (long long)rows2);
    S2D_CHECK_ARG((rows0 == 0 || cloud0) && (rows1 == 0 || cloud1) && (rows2 == 0 || cloud2), "prep_global_noise: null cloud");
    const int64_t total = rows0 + rows1 + rows2;
    if (total == 0) return S2D_OK;
    NoiseArgs a;
    a.cloud[0] = cloud0, a.cloud[1] = cloud1, a.cloud[2] = cloud2;
    a.rows[0] = rows0, a.rows[1] = rows1, a.rows[2] = rows2;
    a.ncols = ncols, a.flip_x = flip_x != 0, a.flip_y = flip_y != 0, a.translate = translate != 0;
    a.rot_cos = rot_cos, a.rot_sin = rot_sin, a.scale = scale;
    a.t[0] = tx, a.t[1] = ty, a.t[2] = tz;
    hipLaunchKernelGGL(prep_noise_kernel, dim3((unsigned)ceil_div(total, PREP_THREADS)), dim3(PREP_THREADS), 0, (hipStream_t)stream, a);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_prep_gather_rows(const float *src, int64_t rows, int ncols, const int64_t *perm, float *dst, s2d_stream_t stream) {
    S2D_CHECK_ARG(ncols >= 1 && ncols <= 16, "prep_gather_rows: %d columns (1..16)", ncols);
    S2D_CHECK_ARG(rows >= 0 && rows <= 3ll * S2D_PREP_MAX_POINTS, "prep_gather_rows: rows %lld", (long long)rows);
    if (rows == 0) return S2D_OK;
    S2D_CHECK_ARG(src && perm && dst && src != dst, "prep_gather_rows: null argument or in-place gather");
    hipLaunchKernelGGL(prep_gather_kernel, dim3((unsigned)ceil_div(rows * ncols, PREP_THREADS)), dim3(PREP_THREADS), 0, (hipStream_t)stream, src, rows,
                       ncols, perm, dst);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" size_t s2d_prep_gt_scratch_bytes(int num_avoid, int num_cand) {
    if (num_avoid < 0 || num_cand < 1 || num_cand > GT_MAX_CAND || num_avoid + num_cand > PREP_MAX_BOXES) return 0;
    return gt_carve(nullptr, num_cand).bytes + 256;
}

extern "C" int s2d_prep_box_collision(const float *corners, int n, const float *qcorners, int k, uint8_t *out, s2d_stream_t stream) {
    S2D_CHECK_ARG(n >= 0 && k >= 0 && (int64_t)n * k <= (int64_t)1 << 24, "prep_box_collision: %d x %d boxes (at most 2^24 pairs)", n, k);
    if (n == 0 || k == 0) return S2D_OK;
    S2D_CHECK_ARG(corners && qcorners && out, "prep_box_collision: null corners or output");
    hipLaunchKernelGGL(prep_collision_kernel, dim3((unsigned)ceil_div((int64_t)n * k, PREP_THREADS)), dim3(PREP_THREADS), 0, (hipStream_t)stream,
                       corners, n, qcorners, k, out);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_prep_gt_select(const float *boxes, int num_avoid, int num_cand, int box_dim, const int32_t *group_ends, int num_groups,
                                  const int32_t *cand_meta, const float *cc_points, int64_t src_rows, int64_t cc_rows, int ncols, void *ws,
                                  size_t ws_bytes, int32_t *header, s2d_stream_t stream) {
    if (int rc = gt_check_sizes("prep_gt_select", num_avoid, num_cand, box_dim, ncols, src_rows, cc_rows)) return rc;
    S2D_CHECK_ARG(num_groups >= 1 && num_groups <= GT_MAX_GROUPS && group_ends, "prep_gt_select: %d groups (1..%d)", num_groups, GT_MAX_GROUPS);
    GtGroups groups;
    groups.n = num_groups;
    for (int g = 0; g < GT_MAX_GROUPS; ++g) groups.end[g] = g < num_groups ? group_ends[g] : num_cand;
    for (int g = 0; g < num_groups; ++g)
        S2D_CHECK_ARG(groups.end[g] >= (g ? groups.end[g - 1] : 0) && groups.end[g] <= num_cand, "prep_gt_select: group ends must not decrease (0..%d)",
                      num_cand);
    S2D_CHECK_ARG(boxes && cand_meta && header, "prep_gt_select: null boxes, candidate table or header");
    S2D_CHECK_ARG(cc_rows == 0 || cc_points, "prep_gt_select: null completed clouds");
    const GtWs w = gt_carve(ws, num_cand);
    if (!ws || ws_bytes < w.bytes) {
        set_error("prep_gt_select: workspace %zu bytes, %zu needed", ws_bytes, w.bytes);
        return S2D_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gt_select_kernel, dim3(1), dim3(PREP_THREADS), 0, st, boxes, num_avoid, num_cand, box_dim, groups, cand_meta, src_rows, cc_rows,
                       w.table, w.range, w.seg, header);
    hipLaunchKernelGGL(gt_count_kernel, dim3(num_cand), dim3(PREP_THREADS), 0, st, num_cand, ncols, cand_meta, cc_points, w.table, w.range, w.seg, header);
    hipLaunchKernelGGL(gt_segments_kernel, dim3(1), dim3(PREP_THREADS), 0, st, num_cand, w.seg, header);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}

extern "C" int s2d_prep_gt_paste(int num_cand, int ncols, const int32_t *cand_meta, const float *src_points, int64_t src_rows, const float *cc_points,
                                 int64_t cc_rows, const void *ws, size_t ws_bytes, const int32_t *header, float *points_out, float *dense_out,
                                 int64_t sampled_rows, float *recon_out, int64_t recon_rows, s2d_stream_t stream) {
    if (int rc = gt_check_sizes("prep_gt_paste", 0, num_cand, 7, ncols, src_rows, cc_rows)) return rc;
    S2D_CHECK_ARG(sampled_rows >= 0 && recon_rows >= 0 && sampled_rows <= S2D_PREP_MAX_POINTS && recon_rows <= S2D_PREP_MAX_POINTS,
                  "prep_gt_paste: output rows %lld / %lld", (long long)sampled_rows, (long long)recon_rows);
    S2D_CHECK_ARG(cand_meta && header, "prep_gt_paste: null candidate table or header");
    S2D_CHECK_ARG((src_rows == 0 || src_points) && (cc_rows == 0 || cc_points), "prep_gt_paste: null stored rows");
    S2D_CHECK_ARG(sampled_rows == 0 || points_out, "prep_gt_paste: null output");
    const GtWs w = gt_carve(const_cast<void *>(ws), num_cand);
    if (!ws || ws_bytes < w.bytes) {
        set_error("prep_gt_paste: workspace %zu bytes, %zu needed", ws_bytes, w.bytes);
        return S2D_ERR_WORKSPACE;
    }
    hipLaunchKernelGGL(gt_paste_kernel, dim3(num_cand), dim3(PREP_THREADS), 0, (hipStream_t)stream, num_cand, ncols, cand_meta, src_points, cc_points,
                       w.table, w.range, w.seg, header, points_out, dense_out, (int)sampled_rows, recon_rows ? recon_out : nullptr, (int)recon_rows);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
