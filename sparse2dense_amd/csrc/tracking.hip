// Center-based multi-object tracker (the reference's PubTracker.step_centertrack, tools/nusc_tracking/pub_tracker.py and
// tools/waymo_tracking/tracker.py, behind transform_box of tools/waymo_tracking/test.py:160-183): greedy closest-centre association after
// moving every detection back along its velocity.  One workgroup of 1024 threads per segment (sequence), all segments in one launch; the
// track lists live on the device, double-buffered (read old, write new), and no result is read by the host.
//
//   stage    thread r owns row r of its segment: centre and velocity into the global frame and `tracking = velocity * -1 * time_lag` in
//            double (kept in registers for the fill), the matching centre float32(ct + float64(float32(tracking))), class and max_diff
//            into LDS; the old tracks' float32 centres and classes into LDS.
//   phase 1  one wave per detection: its best valid track over ALL tracks (key = distance bits << 32 | track index, a wave-wide minimum:
//            the smallest distance, the lowest index on equal distances, as argmin).
//   phase 2  wave 0 walks the detections in input order with the taken mask in registers (lane l holds tracks 64 l .. 64 l + 63): a free
//            choice is taken; a taken one is recomputed over the free tracks.  A detection's best over the free set is its unconstrained
//            best whenever that one is free, so this is the sequential greedy result.
//   phase 3  three in-workgroup scans (matched detections, new detections, surviving old tracks) and the fill in the reference's order.
//
// The float32 distance is sqrt(dx * dx + dy * dy) with every operation rounded on its own (__fmul_rn / __fadd_rn / __fsqrt_rn, and the
// library is built with contraction off).  All counts are integers, there is no atomic and no scalar memory write: two calls on the same
// inputs give the same bits.
#include "s2d_common.h"

namespace s2d {
namespace {

constexpr int TRK_THREADS = 1024;
constexpr int TRK_WAVES = TRK_THREADS / 64;
constexpr int TRK_CAP = S2D_TRACK_MAX_TRACKS;
constexpr int TRK_DETS = S2D_TRACK_MAX_DETS;
constexpr int TRK_PER_THREAD = TRK_CAP / TRK_THREADS;
constexpr unsigned long long TRK_NONE = ~0ull;
static_assert(TRK_DETS == TRK_THREADS, "a thread owns one row of its segment");
static_assert(TRK_CAP == 64 * 64, "the taken mask is one 64-bit word per lane of a wave");

struct TrkState {
    double *ct, *trk;      // [S][TRK_CAP][2]
    int32_t *meta, *head;  // [S][TRK_CAP][4] = class, id, age, active; [S][2] = count, id_count
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

// distance of track centre (tx, ty) from detection centre (dx, dy) as a sortable key, TRK_NONE when it exceeds max_diff (or is no number)
__device__ __forceinline__ unsigned long long pair_key(float tx, float ty, float dx, float dy, float max_diff, int j) {
    const float ex = __fsub_rn(tx, dx), ey = __fsub_rn(ty, dy);
    const float d = __fsqrt_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)));
    if (!(d <= max_diff)) return TRK_NONE;
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;
}

__device__ __forceinline__ int trk_wave_inclusive_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive scan of one int per thread over the 1024 threads; the total in *total
__device__ __forceinline__ int trk_block_scan(int v, int *total, int *lds /*[TRK_WAVES]*/) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int inc = trk_wave_inclusive_scan(v);
    if (lane == 63) lds[wid] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TRK_WAVES; ++w) {
        const int s = lds[w];
        if (w < wid) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__global__ __launch_bounds__(TRK_THREADS) void track_step_kernel(const float *__restrict__ boxes, const int64_t *__restrict__ labels,
                                                                 const float *__restrict__ scores, int rows,
                                                                 const s2d_track_segment *__restrict__ segments,
                                                                 const s2d_track_label *__restrict__ label_table, int num_labels, int max_age,
                                                                 float score_thresh, TrkState old_, TrkState new_,
                                                                 int32_t *__restrict__ tracking_id, int32_t *__restrict__ active) {
    __shared__ float s_tx[TRK_CAP], s_ty[TRK_CAP];
    __shared__ int8_t s_tcls[TRK_CAP];
    __shared__ unsigned long long s_taken[64];
    __shared__ float s_dx[TRK_DETS], s_dy[TRK_DETS], s_dmax[TRK_DETS];
    __shared__ int8_t s_dcls[TRK_DETS];
    __shared__ int s_best[TRK_DETS], s_match[TRK_DETS];
    __shared__ int s_scan[TRK_WAVES];

    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const s2d_track_segment &seg = segments[s];
    int lo = seg.row_lo, hi = seg.row_hi;
    lo = lo < 0 ? 0 : lo > rows ? rows : lo;
    hi = hi < lo ? lo : hi > rows ? rows : hi;
    const int n = hi - lo < TRK_DETS ? hi - lo : TRK_DETS;   // (the host refuses more; rows past the limit are reported as dropped)
    for (int r = lo + n + tid; r < hi; r += TRK_THREADS) {
        tracking_id[r] = -1;
        active[r] = 0;
    }

    const size_t sbase = (size_t)s * TRK_CAP;
    const double *ct_old = old_.ct + sbase * 2, *trk_old = old_.trk + sbase * 2;
    const int32_t *meta_old = old_.meta + sbase * 4;
    double *ct_new = new_.ct + sbase * 2, *trk_new = new_.trk + sbase * 2;
    int32_t *meta_new = new_.meta + sbase * 4;
    int m = old_.head[s * 2 + 0], id_count = old_.head[s * 2 + 1];
    m = m < 0 ? 0 : m > TRK_CAP ? TRK_CAP : m;

    if (seg.skip) {   // the segment's whole slab moves to the other buffer bit for bit; its rows (if any) are reported as dropped
        for (int i = tid; i < TRK_CAP * 2; i += TRK_THREADS) {
            ct_new[i] = ct_old[i];
            trk_new[i] = trk_old[i];
        }
        for (int i = tid; i < TRK_CAP * 4; i += TRK_THREADS) meta_new[i] = meta_old[i];
        if (tid == 0) {
            new_.head[s * 2 + 0] = m;
            new_.head[s * 2 + 1] = id_count;
        }
        if (tid < n) {
            tracking_id[lo + tid] = -1;
            active[lo + tid] = 0;
        }
        return;
    }
    if (seg.first) {   // reset()
        m = 0;
        id_count = 0;
    }
    if (n == 0) {   // a frame without detections: the tracks are cleared, id_count stays
        if (tid == 0) {
            new_.head[s * 2 + 0] = 0;
            new_.head[s * 2 + 1] = id_count;
        }
        return;
    }

    // ---- stage
    for (int j = tid; j < m; j += TRK_THREADS) {
        s_tx[j] = (float)ct_old[j * 2 + 0];
        s_ty[j] = (float)ct_old[j * 2 + 1];
        s_tcls[j] = (int8_t)meta_old[j * 4 + 0];
    }
    double ctx = 0.0, cty = 0.0, trx = 0.0, try_ = 0.0;
    int cls = -1;
    if (tid < n) {
        const int row = lo + tid;
        const int64_t label = labels[row];
        float max_diff = 0.f;
        if (label >= 0 && label < num_labels) {
            cls = label_table[label].cls;
            max_diff = label_table[label].max_diff;
        }
        if (cls >= 0) {
            const float *b = boxes + (size_t)row * 9;
            const double x = b[0], y = b[1], z = b[2], vx = b[6], vy = b[7];
            const double *p = seg.pose;
            ctx = ((p[0] * x + p[1] * y) + p[2] * z) + p[3];
            cty = ((p[4] * x + p[5] * y) + p[6] * z) + p[7];
            trx = ((p[0] * vx + p[1] * vy) * -1.0) * seg.time_lag;
            try_ = ((p[4] * vx + p[5] * vy) * -1.0) * seg.time_lag;
            s_dx[tid] = (float)(ctx + (double)(float)trx);
            s_dy[tid] = (float)(cty + (double)(float)try_);
        } else {
            cls = -1;
        }
        s_dmax[tid] = max_diff;
        s_dcls[tid] = (int8_t)cls;
        s_match[tid] = -1;
    }
    __syncthreads();

    // ---- phase 1: the unconstrained best track of every detection
    for (int r = wid; r < n; r += TRK_WAVES) {
        const int c = s_dcls[r];
        if (c < 0) continue;
        const float dx = s_dx[r], dy = s_dy[r], dmax = s_dmax[r];
        unsigned long long key = TRK_NONE;
        for (int j = lane; j < m; j += 64) {
            if (s_tcls[j] != c) continue;
            const unsigned long long k = pair_key(s_tx[j], s_ty[j], dx, dy, dmax, j);
            key = k < key ? k : key;
        }
        key = wave_min_u64(key);
        if (lane == 0) s_best[r] = key == TRK_NONE ? -1 : (int)(unsigned)(key & 0xffffffffull);
    }
    __syncthreads();

    // ---- phase 2: detections in input order
    if (wid == 0) {
        unsigned long long taken = 0;   // tracks 64 * lane .. 64 * lane + 63
        for (int r = 0; r < n; ++r) {
            const int c = __builtin_amdgcn_readfirstlane((int)s_dcls[r]);   // (the same address in every lane: made uniform for the compiler too)
            if (c < 0) continue;
            int b = __builtin_amdgcn_readfirstlane(s_best[r]);
            const int probe = b < 0 ? 0 : b;
            const bool lost = ((__shfl(taken, probe >> 6, 64) >> (probe & 63)) & 1ull) != 0;
            if (b >= 0 && lost) {
                const float dx = s_dx[r], dy = s_dy[r], dmax = s_dmax[r];
                unsigned long long key = TRK_NONE;
                for (int k = 0; k * 64 < m; ++k) {
                    const unsigned long long word = __shfl(taken, k, 64);
                    const int j = k * 64 + lane;
                    if (j < m && !((word >> lane) & 1ull) && s_tcls[j] == c) {
                        const unsigned long long q = pair_key(s_tx[j], s_ty[j], dx, dy, dmax, j);
                        key = q < key ? q : key;
                    }
                }
                key = wave_min_u64(key);
                b = key == TRK_NONE ? -1 : (int)(unsigned)(key & 0xffffffffull);
            }
            if (b >= 0 && lane == (b >> 6)) taken |= 1ull << (b & 63);
            if (lane == 0) s_match[r] = b;
        }
        s_taken[lane] = taken;
    }
    __syncthreads();

    // ---- phase 3: counts, scans, fill
    const int match = tid < n ? s_match[tid] : -1;
    const bool kept = tid < n && cls >= 0;
    const int is_matched = kept && match >= 0;
    const int is_new = kept && match < 0 && (score_thresh < 0.f || scores[lo + tid] > score_thresh);
    int survives[TRK_PER_THREAD];
    int n_survive = 0;
#pragma unroll
    for (int t = 0; t < TRK_PER_THREAD; ++t) {
        const int j = tid * TRK_PER_THREAD + t;
        survives[t] = j < m && !((s_taken[j >> 6] >> (j & 63)) & 1ull) && meta_old[j * 4 + 2] < max_age;
        n_survive += survives[t];
    }
    int total_matched, total_new, total_old;
    const int pos_matched = trk_block_scan(is_matched, &total_matched, s_scan);
    const int pos_new = trk_block_scan(is_new, &total_new, s_scan);
    int pos_old = trk_block_scan(n_survive, &total_old, s_scan);

    if (tid < n) {
        int id = -1, act = 0, pos = -1;
        if (is_matched) {
            id = meta_old[match * 4 + 1];
            act = meta_old[match * 4 + 3] + 1;
            pos = pos_matched;
        } else if (is_new) {
            id = id_count + pos_new + 1;
            act = 1;
            pos = total_matched + pos_new;
        }
        tracking_id[lo + tid] = id;
        active[lo + tid] = act;
        if (pos >= 0 && pos < TRK_CAP) {
            ct_new[pos * 2 + 0] = ctx;
            ct_new[pos * 2 + 1] = cty;
            trk_new[pos * 2 + 0] = trx;
            trk_new[pos * 2 + 1] = try_;
            meta_new[pos * 4 + 0] = cls;
            meta_new[pos * 4 + 1] = id;
            meta_new[pos * 4 + 2] = 1;
            meta_new[pos * 4 + 3] = act;
        }
    }
    pos_old += total_matched + total_new;
#pragma unroll
    for (int t = 0; t < TRK_PER_THREAD; ++t) {
        if (!survives[t]) continue;
        const int j = tid * TRK_PER_THREAD + t;
        if (pos_old < TRK_CAP) {   // the track moves forward by the motion of its last detection: ct - tracking
            ct_new[pos_old * 2 + 0] = ct_old[j * 2 + 0] - trk_old[j * 2 + 0];
            ct_new[pos_old * 2 + 1] = ct_old[j * 2 + 1] - trk_old[j * 2 + 1];
            trk_new[pos_old * 2 + 0] = trk_old[j * 2 + 0];
            trk_new[pos_old * 2 + 1] = trk_old[j * 2 + 1];
            meta_new[pos_old * 4 + 0] = meta_old[j * 4 + 0];
            meta_new[pos_old * 4 + 1] = meta_old[j * 4 + 1];
            meta_new[pos_old * 4 + 2] = meta_old[j * 4 + 2] + 1;
            meta_new[pos_old * 4 + 3] = 0;
        }
        ++pos_old;
    }
    if (tid == 0) {
        const int count = total_matched + total_new + total_old;
        new_.head[s * 2 + 0] = count < TRK_CAP ? count : TRK_CAP;
        new_.head[s * 2 + 1] = id_count + total_new;
    }
}

}  // namespace
}  // namespace s2d

using namespace s2d;

extern "C" int s2d_track_step(const float *boxes, const int64_t *labels, const float *scores, int64_t rows, int num_segments,
                              const s2d_track_segment *segments, const s2d_track_label *label_table, int num_labels, int max_age,
                              float score_thresh, const double *ct_old, const double *tracking_old, const int32_t *meta_old,
                              const int32_t *head_old, double *ct_new, double *tracking_new, int32_t *meta_new, int32_t *head_new,
                              int32_t *tracking_id, int32_t *active, s2d_stream_t stream) {
    S2D_CHECK_ARG(num_segments >= 1 && num_segments <= S2D_TRACK_MAX_SEGMENTS, "track_step: %d segments (1..%d)", num_segments,
                  S2D_TRACK_MAX_SEGMENTS);
    S2D_CHECK_ARG(rows >= 0 && rows <= (int64_t)S2D_TRACK_MAX_SEGMENTS * S2D_TRACK_MAX_DETS, "track_step: %lld rows (at most %d per segment)",
                  (long long)rows, S2D_TRACK_MAX_DETS);
    S2D_CHECK_ARG(num_labels >= 1 && num_labels <= 127 && max_age >= 0, "track_step: %d labels (1..127), max_age %d (>= 0)", num_labels, max_age);
    S2D_CHECK_ARG(segments && label_table, "track_step: null segment or label table");
    S2D_CHECK_ARG(rows == 0 || (boxes && labels && scores && tracking_id && active), "track_step: null boxes, labels, scores or row outputs");
    S2D_CHECK_ARG(ct_old && tracking_old && meta_old && head_old && ct_new && tracking_new && meta_new && head_new, "track_step: null state buffer");
    S2D_CHECK_ARG(ct_old != ct_new && tracking_old != tracking_new && meta_old != meta_new && head_old != head_new,
                  "track_step: the old and the new state must be different buffers");
    const TrkState old_{const_cast<double *>(ct_old), const_cast<double *>(tracking_old), const_cast<int32_t *>(meta_old),
                        const_cast<int32_t *>(head_old)};
    const TrkState new_{ct_new, tracking_new, meta_new, head_new};
    hipLaunchKernelGGL(track_step_kernel, dim3(num_segments), dim3(TRK_THREADS), 0, (hipStream_t)stream, boxes, labels, scores, (int)rows, segments,
                       label_table, num_labels, max_age, score_thresh, old_, new_, tracking_id, active);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
