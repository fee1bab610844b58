// The per-anchor arithmetic of MultiGroupHead.predict shared by anchor_decode_kernel (anchor_head.hip: every anchor, dense output) and the
// candidate kernels of anchor_predict.hip: the library is built with -ffp-contract=off, so both give the same bits.
#pragma once
#include "s2d_common.h"

#include <math.h>

namespace s2d {

// maximum over the classes of sigmoid(logit) and its class (mg_head.py:838-849): the first maximum wins a tie
__device__ __forceinline__ float anchor_class_max(const float *__restrict__ logits, int classes, int &arg) {
    float best = 0.f;
    arg = 0;
    for (int j = 0; j < classes; ++j) {
        const float x = logits[j];
        const float e = expf(-fabsf(x));
        const float p = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        if (j == 0 || p > best) {
            best = p;
            arg = j;
        }
    }
    return best;
}

// second_box_decode (det3d/core/bbox/box_torch_ops.py:87-150) of one encoding t[7] on its anchor an[7] -> (x, y, z, w, l, h, r)
__device__ __forceinline__ void anchor_box_decode(const float *__restrict__ t, const float *__restrict__ an, float o[7]) {
    const float diagonal = sqrtf(an[4] * an[4] + an[3] * an[3]);
    o[0] = t[0] * diagonal + an[0];
    o[1] = t[1] * diagonal + an[1];
    o[2] = t[2] * an[5] + an[2];
    o[3] = expf(t[3]) * an[3];
    o[4] = expf(t[4]) * an[4];
    o[5] = expf(t[5]) * an[5];
    o[6] = t[6] + an[6];
}

}  // namespace s2d
