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
//
// Two entries over one body (track_segment_step): s2d_track_step takes packed rows, a segment table with the row ranges and the time lag,
// and the old / new halves chosen by the host; s2d_track_step_static takes padded rows with their counts on the device, forms the time lag
// from a stamp kept on the device and keeps the parity of the halves there, so one recorded launch advances the state at every replay.
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

struct TrkLds {
    float tx[TRK_CAP], ty[TRK_CAP];
    int8_t tcls[TRK_CAP];
    unsigned long long taken[64];
    float dx[TRK_DETS], dy[TRK_DETS], dmax[TRK_DETS];
    int8_t dcls[TRK_DETS];
    int best[TRK_DETS], match[TRK_DETS];
    int scan[TRK_WAVES];
};

// One step of one segment that is not skipped, by its whole workgroup: the body both kernels share, so that every decision and every
// double comes from the same code.  boxes / labels / scores / tracking_id / active point at the segment's first row, n (0 .. TRK_DETS,
// uniform) is its row count; m old tracks (clamped to 0 .. TRK_CAP) are read from *_old and the new list is written to *_new and
// head_new[2] = count, id_count.  Rows 0 .. n - 1 of tracking_id / active are written unless n == 0.
__device__ __forceinline__ void track_segment_step(TrkLds &lds, const float *__restrict__ boxes, const int64_t *__restrict__ labels,
                                                   const float *__restrict__ scores, int n, const double *__restrict__ pose, double time_lag,
                                                   int first, const s2d_track_label *__restrict__ label_table, int num_labels, int max_age,
                                                   float score_thresh, const double *ct_old, const double *trk_old, const int32_t *meta_old, int m,
                                                   int id_count, double *ct_new, double *trk_new, int32_t *meta_new, int32_t *head_new,
                                                   int32_t *__restrict__ tracking_id, int32_t *__restrict__ active) {
    float *s_tx = lds.tx, *s_ty = lds.ty, *s_dx = lds.dx, *s_dy = lds.dy, *s_dmax = lds.dmax;
    int8_t *s_tcls = lds.tcls, *s_dcls = lds.dcls;
    unsigned long long *s_taken = lds.taken;
    int *s_best = lds.best, *s_match = lds.match, *s_scan = lds.scan;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    if (first) {   // reset()
        m = 0;
        id_count = 0;
    }
    if (n == 0) {   // a frame without detections: the tracks are cleared, id_count stays
        if (tid == 0) {
            head_new[0] = 0;
            head_new[1] = id_count;
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
        const int row = tid;
        const int64_t label = labels[row];
        float max_diff = 0.f;
        if (label >= 0 && label < num_labels) {
            cls = label_table[label].cls;
            max_diff = label_table[label].max_diff;
        }
        if (cls >= 0) {
            const float *b = boxes + (size_t)row * 9;
            const double x = b[0], y = b[1], z = b[2], vx = b[6], vy = b[7];
            const double *p = pose;
            ctx = ((p[0] * x + p[1] * y) + p[2] * z) + p[3];
            cty = ((p[4] * x + p[5] * y) + p[6] * z) + p[7];
            trx = ((p[0] * vx + p[1] * vy) * -1.0) * time_lag;
            try_ = ((p[4] * vx + p[5] * vy) * -1.0) * time_lag;
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
    const int is_new = kept && match < 0 && (score_thresh < 0.f || scores[tid] > score_thresh);
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
        tracking_id[tid] = id;
        active[tid] = act;
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
        head_new[0] = count < TRK_CAP ? count : TRK_CAP;
        head_new[1] = id_count + total_new;
    }
}

__global__ __launch_bounds__(TRK_THREADS) void track_step_kernel(const float *__restrict__ boxes, const int64_t *__restrict__ labels,
                                                                 const float *__restrict__ scores, int rows,
                                                                 const s2d_track_segment *__restrict__ segments,
                                                                 const s2d_track_label *__restrict__ label_table, int num_labels, int max_age,
                                                                 float score_thresh, TrkState old_, TrkState new_,
                                                                 int32_t *__restrict__ tracking_id, int32_t *__restrict__ active) {
    __shared__ TrkLds lds;
    const int s = blockIdx.x, tid = threadIdx.x;
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
    int m = old_.head[s * 2 + 0];
    const int id_count = old_.head[s * 2 + 1];
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
    track_segment_step(lds, boxes + (size_t)lo * 9, labels + lo, scores + lo, n, seg.pose, seg.time_lag, seg.first, label_table, num_labels, max_age,
                       score_thresh, ct_old, trk_old, meta_old, m, id_count, ct_new, trk_new, meta_new, new_.head + s * 2, tracking_id + lo,
                       active + lo);
}

// The static step: padded rows (segment s owns rows s * cap .. s * cap + clamp(counts[s], 0, cap) - 1; nothing behind them is read), the
// frame block, the previous stamp and the buffer parity all read from device memory, so that a launch recorded once advances the state at
// every replay.  Half parity[s] of the doubled state is the old list, the other half the new one; thread 0 flips parity[s] after the fill.
// A skipped segment keeps parity, state and prev_stamp (no slab copy).  All cap rows of the outputs are written at every call.
__global__ __launch_bounds__(TRK_THREADS) void track_step_static_kernel(const float *__restrict__ boxes, const int64_t *__restrict__ labels,
                                                                        const float *__restrict__ scores, const int32_t *__restrict__ counts,
                                                                        int num_segments, int cap, const s2d_track_frame *__restrict__ frames,
                                                                        const s2d_track_label *__restrict__ label_table, int num_labels,
                                                                        int max_age, float score_thresh, TrkState st, int32_t *parity,
                                                                        double *prev_stamp, int32_t *__restrict__ tracking_id,
                                                                        int32_t *__restrict__ active) {
    __shared__ TrkLds lds;
    const int s = blockIdx.x, tid = threadIdx.x;
    const s2d_track_frame &frame = frames[s];
    int n = counts[s];
    n = n < 0 ? 0 : n > cap ? cap : n;
    const int skip = frame.skip, first = frame.first;
    const int p = parity[s] & 1;
    const double stamp = frame.stamp;
    const double lag = first ? 0.0 : stamp - prev_stamp[s];
    __syncthreads();   // every thread has read parity[s] and prev_stamp[s] before thread 0 writes them

    const size_t row0 = (size_t)s * cap;
    if (tid < cap && (skip || tid >= n)) {   // the padding, and every row of a skipped segment
        tracking_id[row0 + tid] = -1;
        active[row0 + tid] = 0;
    }
    if (skip) return;

    const size_t half = (size_t)num_segments * TRK_CAP, obase = (size_t)p * half + (size_t)s * TRK_CAP,
                 nbase = (size_t)(1 - p) * half + (size_t)s * TRK_CAP;
    const int32_t *head_old = st.head + ((size_t)p * num_segments + s) * 2;
    int32_t *head_new = st.head + ((size_t)(1 - p) * num_segments + s) * 2;
    int m = head_old[0];
    const int id_count = head_old[1];
    m = m < 0 ? 0 : m > TRK_CAP ? TRK_CAP : m;
    track_segment_step(lds, boxes + row0 * 9, labels + row0, scores + row0, n, frame.pose, lag, first, label_table, num_labels, max_age, score_thresh,
                       st.ct + obase * 2, st.trk + obase * 2, st.meta + obase * 4, m, id_count, st.ct + nbase * 2, st.trk + nbase * 2,
                       st.meta + nbase * 4, head_new, tracking_id + row0, active + row0);
    if (tid == 0) {
        parity[s] = 1 - p;
        prev_stamp[s] = stamp;
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

extern "C" int s2d_track_step_static(const float *boxes, const int64_t *labels, const float *scores, const int32_t *counts, int num_segments,
                                     int cap, const s2d_track_frame *frames, const s2d_track_label *label_table, int num_labels, int max_age,
                                     float score_thresh, double *ct, double *tracking, int32_t *meta, int32_t *head, int32_t *parity,
                                     double *prev_stamp, int32_t *tracking_id, int32_t *active, s2d_stream_t stream) {
    S2D_CHECK_ARG(num_segments >= 1 && num_segments <= S2D_TRACK_MAX_SEGMENTS, "track_step_static: %d segments (1..%d)", num_segments,
                  S2D_TRACK_MAX_SEGMENTS);
    S2D_CHECK_ARG(cap >= 1 && cap <= S2D_TRACK_MAX_DETS, "track_step_static: cap %d (1..%d rows per segment)", cap, S2D_TRACK_MAX_DETS);
    S2D_CHECK_ARG(num_labels >= 1 && num_labels <= 127, "track_step_static: %d labels (1..127)", num_labels);
    S2D_CHECK_ARG(max_age >= 0 && (int64_t)cap * ((int64_t)max_age + 1) <= S2D_TRACK_MAX_TRACKS,
                  "track_step_static: cap %d x (max_age %d + 1) = %lld tracks (at most %d per segment)", cap, max_age,
                  (long long)cap * ((long long)max_age + 1), S2D_TRACK_MAX_TRACKS);
    S2D_CHECK_ARG(boxes && labels && scores && counts && tracking_id && active, "track_step_static: null boxes, labels, scores, counts or row outputs");
    S2D_CHECK_ARG(frames && label_table, "track_step_static: null frame block or label table");
    S2D_CHECK_ARG(ct && tracking && meta && head && parity && prev_stamp, "track_step_static: null state buffer, parity or prev_stamp");
    const TrkState st{ct, tracking, meta, head};
    hipLaunchKernelGGL(track_step_static_kernel, dim3(num_segments), dim3(TRK_THREADS), 0, (hipStream_t)stream, boxes, labels, scores, counts,
                       num_segments, cap, frames, label_table, num_labels, max_age, score_thresh, st, parity, prev_stamp, tracking_id, active);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
