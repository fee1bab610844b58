// s2d_segment_topk: the first k columns of the stable descending sort of every row of a score matrix, one workgroup per row, without
// sorting the row.  It stands where CenterHead.predict's torch.sort stood (center_predict.py): a [24, 32 400] score map has about 300
// passing cells per row and at most nms_pre_max_size of them are used.
//   keys      a float becomes a 32-bit key that orders as the float does (-0.0 folded onto +0.0, so the two compare equal); an element
//             is the 64-bit item (key, ~index): a larger item is a larger value or, among equal values, a lower index.  All items of a
//             row differ, so any sort of them is the stable descending sort.
//   select    (rows longer than k) three histogram passes over the row - 11, 11 and 10 key bits, LDS histograms - find the key T of rank
//             k and the number of elements above it; a fourth pass puts every element above T into LDS (any order: they are sorted
//             below) and counts the elements equal to T per wave, each wave owning one contiguous span of the row; a fifth writes the
//             lowest-index k - above elements equal to T behind them, each wave at the base its predecessors' counts give it.
//   sort      bitonic sort of the at most 4096 items in LDS, then rank r's index and value (read back from the row: the key has lost
//             the sign of a zero) go to order / score_sorted.
// Workgroups do not communicate; all state is in LDS and in the outputs.  The row is read with 16-byte loads wherever a group of four
// elements lies on a 16-byte boundary inside the row (any row base and stride), else element by element.
#include "s2d_common.h"

namespace s2d {

constexpr int TK_THREADS = 1024, TK_WAVES = TK_THREADS / 64, TK_MAX_K = 4096, TK_BINS = 2048;

__device__ __forceinline__ uint32_t topk_key(float x) {
    uint32_t u = __float_as_uint(x);
    if (x == 0.f) u = 0u;   // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long topk_item(uint32_t key, int64_t index) {
    return ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)index;
}

// The row as groups of four elements: group v holds elements 4 v - pad .. 4 v - pad + 3, pad = the row base's distance (in floats) from
// the 16-byte boundary below it, so every group that lies inside the row is one aligned 16-byte load.
struct RowView {
    const float *row;
    int64_t len, groups;
    int pad;
};

__device__ __forceinline__ RowView row_view(const float *row, int64_t len) {
    RowView r;
    r.row = row;
    r.len = len;
    r.pad = (int)(((uintptr_t)row >> 2) & 3);
    r.groups = (len + r.pad + 3) / 4;
    return r;
}

// keys of group v; bit j of the result is set where element j of the group exists (first[0] = index of element 0, may be negative)
__device__ __forceinline__ unsigned load_group(const RowView &r, int64_t v, uint32_t key[4], int64_t &first) {
    first = 4 * v - r.pad;
    if (first >= 0 && first + 4 <= r.len) {
        const float4 f = *reinterpret_cast<const float4 *>(r.row + first);
        key[0] = topk_key(f.x);
        key[1] = topk_key(f.y);
        key[2] = topk_key(f.z);
        key[3] = topk_key(f.w);
        return 0xFu;
    }
    unsigned valid = 0u;
    for (int j = 0; j < 4; ++j) {
        const int64_t e = first + j;
        key[j] = 0u;
        if (e >= 0 && e < r.len) {
            key[j] = topk_key(r.row[e]);
            valid |= 1u << j;
        }
    }
    return valid;
}

// exclusive prefix of v over the workgroup in thread order; `total` = the sum.  wave_sums: TK_WAVES ints of LDS, free again on return.
__device__ __forceinline__ int block_exclusive_scan(int v, int *wave_sums, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int i = 0; i < TK_WAVES; ++i) {
        const int s = wave_sums[i];
        if (i < wave) base += s;
        total += s;
    }
    __syncthreads();
    return base + inc - v;
}

struct SelectState {
    uint32_t prefix;   // the key bits fixed so far (right-aligned)
    int rank;          // rank (1-based, from the top) of the wanted element among the elements that match `prefix`
    int above;         // elements placed so far by the fourth pass
};

// One histogram pass: among the elements whose key >> (shift + bits) equals st.prefix, find the digit (key >> shift) & (2^bits - 1) that
// holds rank st.rank, and move both into st.  A thread adds a run of equal digits with one atomic: a row of one repeated value (an
// untrained heat map, or -inf on 99 % of a trained one) would otherwise put every element on one LDS word.
__device__ __forceinline__ void select_pass(const RowView &r, int shift, int bits, bool first_pass, int *hist, int *wave_sums, SelectState &st) {
    const int bins = 1 << bits;
    for (int i = threadIdx.x; i < TK_BINS; i += TK_THREADS) hist[i] = 0;
    __syncthreads();
    const uint32_t prefix = st.prefix;
    int last = -1, run = 0;
    for (int64_t v = threadIdx.x; v < r.groups; v += TK_THREADS) {
        uint32_t key[4];
        int64_t first;
        const unsigned valid = load_group(r, v, key, first);
        for (int j = 0; j < 4; ++j) {
            if (!((valid >> j) & 1u)) continue;
            if (!first_pass && (key[j] >> (shift + bits)) != prefix) continue;
            const int digit = (int)((key[j] >> shift) & (uint32_t)(bins - 1));
            if (digit != last) {
                if (run) atomicAdd(&hist[last], run);
                last = digit;
                run = 0;
            }
            ++run;
        }
    }
    if (run) atomicAdd(&hist[last], run);
    __syncthreads();
    // thread t owns the digits bins - 1 - 2 t and bins - 2 - 2 t: thread order is descending digit order
    const int hi = bins - 1 - 2 * (int)threadIdx.x, lo = hi - 1;
    const int n_hi = hi >= 0 ? hist[hi] : 0, n_lo = lo >= 0 ? hist[lo] : 0;
    int total;
    const int before = block_exclusive_scan(n_hi + n_lo, wave_sums, total);
    const int rank = st.rank;
    __syncthreads();   // every thread has read st
    if (before < rank && rank <= before + n_hi + n_lo) {   // exactly one thread: the histogram holds at least `rank` elements
        const bool in_hi = rank <= before + n_hi;
        st.prefix = (prefix << bits) | (uint32_t)(in_hi ? hi : lo);
        st.rank = rank - before - (in_hi ? 0 : n_hi);
    }
    __syncthreads();
}

__global__ __launch_bounds__(TK_THREADS) void segment_topk_kernel(const float *__restrict__ score, int64_t row_len, int64_t row_stride, int k,
                                                                  const int32_t *__restrict__ passed, int64_t *__restrict__ order,
                                                                  float *__restrict__ score_sorted, int64_t out_stride,
                                                                  int32_t *__restrict__ offsets, int32_t *__restrict__ counts,
                                                                  int32_t *__restrict__ overflow) {
    __shared__ unsigned long long items[TK_MAX_K];
    __shared__ int hist[TK_BINS];
    __shared__ int wave_sums[TK_WAVES], wave_equal[TK_WAVES];
    __shared__ SelectState st;
    const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0 && passed) {
        const int p = passed[seg];
        offsets[seg] = seg * k;
        counts[seg] = p < 0 ? 0 : (p < k ? p : k);
        overflow[seg] = p > k;
    }
    const RowView r = row_view(score + (int64_t)seg * row_stride, row_len);
    const int n = (int)(row_len < k ? row_len : k);
    if (n == 0) return;
    int pow2 = 1;
    while (pow2 < n) pow2 <<= 1;
    for (int i = n + tid; i < pow2; i += TK_THREADS) items[i] = 0ull;   // below every item of the row (an index is < 2^32 - 1)

    if (row_len <= k) {
        for (int64_t v = tid; v < r.groups; v += TK_THREADS) {
            uint32_t key[4];
            int64_t first;
            const unsigned valid = load_group(r, v, key, first);
            for (int j = 0; j < 4; ++j)
                if ((valid >> j) & 1u) items[first + j] = topk_item(key[j], first + j);
        }
    } else {
        if (tid == 0) {
            st.prefix = 0u;
            st.rank = k;
            st.above = 0;
        }
        __syncthreads();
        select_pass(r, 21, 11, true, hist, wave_sums, st);
        select_pass(r, 10, 11, false, hist, wave_sums, st);
        select_pass(r, 0, 10, false, hist, wave_sums, st);
        const uint32_t T = st.prefix;
        const int need_equal = st.rank, above = k - need_equal;   // 1 <= need_equal <= k
        // wave w owns the groups [w * span, (w + 1) * span): its elements precede those of wave w + 1 in the row
        const int64_t span = (r.groups + TK_WAVES - 1) / TK_WAVES;
        const int64_t v_begin = (int64_t)wave * span, v_end = v_begin + span < r.groups ? v_begin + span : r.groups;
        int equal = 0;
        for (int64_t v = v_begin + lane; v < v_end; v += 64) {
            uint32_t key[4];
            int64_t first;
            const unsigned valid = load_group(r, v, key, first);
            for (int j = 0; j < 4; ++j) {
                if (!((valid >> j) & 1u)) continue;
                if (key[j] > T) {
                    const int slot = atomicAdd(&st.above, 1);
                    if (slot < above) items[slot] = topk_item(key[j], first + j);   // (always: `above` is their number)
                } else if (key[j] == T) {
                    ++equal;
                }
            }
        }
        for (int d = 32; d > 0; d >>= 1) equal += __shfl_xor(equal, d, 64);
        if (lane == 0) wave_equal[wave] = equal;
        __syncthreads();
        int base = 0;
        for (int i = 0; i < wave; ++i) base += wave_equal[i];
        // (wave-uniform) the elements equal to T of this wave take the places base .. base + equal - 1 among the row's; the first
        // need_equal places are kept
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int64_t v0 = v_begin; v0 < v_end && base < need_equal; v0 += 64) {
            const int64_t v = v0 + lane;
            uint32_t key[4] = {0u, 0u, 0u, 0u};
            int64_t first = 0;
            const unsigned valid = v < v_end ? load_group(r, v, key, first) : 0u;
            int mine = 0, before = 0, all = 0;
            bool eq[4];
            for (int j = 0; j < 4; ++j) {
                eq[j] = ((valid >> j) & 1u) && key[j] == T;
                const unsigned long long b = __ballot(eq[j]);
                before += __popcll(b & below);
                all += __popcll(b);
            }
            for (int j = 0; j < 4; ++j) {
                if (!eq[j]) continue;
                const int place = base + before + mine;
                if (place < need_equal) items[above + place] = topk_item(T, first + j);
                ++mine;
            }
            base += all;
        }
    }

    // bitonic sort, descending
    for (int size = 2; size <= pow2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = tid; i < pow2 / 2; i += TK_THREADS) {
                const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo + stride;
                const bool descending = (lo & size) == 0;
                const unsigned long long a = items[lo], b = items[hi];
                if ((a < b) == descending) {
                    items[lo] = b;
                    items[hi] = a;
                }
            }
        }
    }
    __syncthreads();
    for (int rank = tid; rank < n; rank += TK_THREADS) {
        int64_t index = (int64_t)(uint32_t)~(uint32_t)items[rank];
        if (index >= row_len) index = row_len - 1;   // (cannot happen: every item came from the row)
        order[(int64_t)seg * out_stride + rank] = index;
        score_sorted[(int64_t)seg * out_stride + rank] = r.row[index];
    }
}

}  // namespace s2d

using namespace s2d;

extern "C" int s2d_segment_topk(const float *score, int segments, int64_t row_len, int64_t row_stride, int k, const int32_t *passed, int64_t *order,
                                float *score_sorted, int64_t out_stride, int32_t *offsets, int32_t *counts, int32_t *overflow, s2d_stream_t stream) {
    S2D_CHECK_ARG(segments >= 0 && segments <= 65535, "segment_topk: %d segments (0..65535)", segments);
    S2D_CHECK_ARG(k >= 1 && k <= TK_MAX_K, "segment_topk: k %d (1..%d)", k, TK_MAX_K);
    S2D_CHECK_ARG(row_len >= 0 && row_len <= (1ll << 20), "segment_topk: row_len %lld (0..2^20)", (long long)row_len);
    S2D_CHECK_ARG(row_stride >= row_len, "segment_topk: row_stride %lld below row_len %lld", (long long)row_stride, (long long)row_len);
    S2D_CHECK_ARG(out_stride >= (row_len < k ? row_len : k), "segment_topk: out_stride %lld below min(k, row_len)", (long long)out_stride);
    if (segments == 0) return S2D_OK;
    S2D_CHECK_ARG(!passed || (offsets && counts && overflow), "segment_topk: pass counts without a segment table to write");
    if (row_len == 0 && !passed) return S2D_OK;
    S2D_CHECK_ARG(row_len == 0 || (score && order && score_sorted), "segment_topk: null argument");
    hipLaunchKernelGGL(segment_topk_kernel, dim3((unsigned)segments), dim3(TK_THREADS), 0, (hipStream_t)stream, score, row_len, row_stride, k, passed,
                       order, score_sorted, out_stride, offsets, counts, overflow);
    S2D_LAUNCH_CHECK();
    return S2D_OK;
}
