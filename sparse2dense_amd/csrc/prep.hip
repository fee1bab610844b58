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
