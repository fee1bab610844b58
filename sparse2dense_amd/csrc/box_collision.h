// The pair test of the GT-database sampler, box_collision_test (det3d/core/sampler/preprocess.py:922-1005), shared by the collision-matrix
// kernel and the select kernel of prep.hip: the library is built with -ffp-contract=off, so both give the same bits.
// The `ret[i, j] is True / is False` comparisons are read by value (numba's reading): a box wholly inside the other collides.
#pragma once
#include "s2d_common.h"

#include <math.h>

namespace s2d {

// BEV corners of one box, center_to_corner_box2d (box_np_ops.py:55-85,207-220,265-285): (-, -), (-, +), (+, +), (+, -) halves of the size,
// x' = x cos r + y sin r, y' = -x sin r + y cos r, plus the centre; cos and sin in double from the fp32 yaw, rounded to fp32.
// c[8] = x0 y0 .. x3 y3, su[4] = the stand-up box (min x, min y, max x, max y).
__device__ __forceinline__ void bev_corners_of(const float *__restrict__ box, int box_dim, float *c, float *su) {
    const double r = (double)box[box_dim - 1];
    const float cs = (float)cos(r), sn = (float)sin(r);
    const float hx[4] = {-0.5f, -0.5f, 0.5f, 0.5f}, hy[4] = {-0.5f, 0.5f, 0.5f, -0.5f};
    float lo_x = 0.f, lo_y = 0.f, hi_x = 0.f, hi_y = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float x = box[3] * hx[k], y = box[4] * hy[k];
        const float px = (x * cs + y * sn) + box[0], py = (x * -sn + y * cs) + box[1];
        c[2 * k] = px, c[2 * k + 1] = py;
        lo_x = k ? fminf(lo_x, px) : px, hi_x = k ? fmaxf(hi_x, px) : px;
        lo_y = k ? fminf(lo_y, py) : py, hi_y = k ? fmaxf(hi_y, py) : py;
    }
    su[0] = lo_x, su[1] = lo_y, su[2] = hi_x, su[3] = hi_y;
}

__device__ __forceinline__ void standup_of(const float *c, float *su) {
    su[0] = fminf(fminf(c[0], c[2]), fminf(c[4], c[6])), su[1] = fminf(fminf(c[1], c[3]), fminf(c[5], c[7]));
    su[2] = fmaxf(fmaxf(c[0], c[2]), fmaxf(c[4], c[6])), su[3] = fmaxf(fmaxf(c[1], c[3]), fmaxf(c[5], c[7]));
}

// every corner of q strictly inside b (the clockwise cross products, `cross >= 0` fails)
__device__ __forceinline__ bool box_holds_corners(const float *b, const float *q) {
    for (int l = 0; l < 4; ++l)
        for (int k = 0; k < 4; ++k) {
            const int k1 = (k + 1) & 3;
            const float v0 = -(b[2 * k] - b[2 * k1]), v1 = -(b[2 * k + 1] - b[2 * k1 + 1]);
            float cross = v1 * (b[2 * k] - q[2 * l]);
            cross -= v0 * (b[2 * k + 1] - q[2 * l + 1]);
            if (cross >= 0.f) return false;
        }
    return true;
}

// ret[i][j] of box_collision_test(boxes, qboxes): b = boxes[i], q = qboxes[j] (corners and stand-up boxes)
__device__ __forceinline__ bool box_pair_collides(const float *b, const float *bs, const float *q, const float *qs) {
    const float iw = fminf(bs[2], qs[2]) - fmaxf(bs[0], qs[0]);
    if (!(iw > 0.f)) return false;
    const float ih = fminf(bs[3], qs[3]) - fmaxf(bs[1], qs[1]);
    if (!(ih > 0.f)) return false;
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        const float a0 = b[2 * k], a1 = b[2 * k + 1], b0 = b[2 * k1], b1 = b[2 * k1 + 1];
        for (int l = 0; l < 4; ++l) {
            const int l1 = (l + 1) & 3;
            const float c0 = q[2 * l], c1 = q[2 * l + 1], d0 = q[2 * l1], d1 = q[2 * l1 + 1];
            const bool acd = (d1 - a1) * (c0 - a0) > (c1 - a1) * (d0 - a0);
            const bool bcd = (d1 - b1) * (c0 - b0) > (c1 - b1) * (d0 - b0);
            if (acd != bcd) {
                const bool abc = (c1 - a1) * (b0 - a0) > (b1 - a1) * (c0 - a0);
                const bool abd = (d1 - a1) * (b0 - a0) > (b1 - a1) * (d0 - a0);
                if (abc != abd) return true;
            }
        }
    }
    return box_holds_corners(b, q) || box_holds_corners(q, b);
}

}  // namespace s2d
