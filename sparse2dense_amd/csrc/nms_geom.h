// Rotated-rectangle overlap geometry shared by the NMS kernels (nms.hip, center_predict.hip): see nms.hip for the reference lines.
#pragma once
#include "s2d_common.h"

namespace s2d {

struct P2 {
    float x, y;
};

__host__ __device__ inline float cross2(const P2 &a, const P2 &b, const P2 &o) { return (a.x - o.x) * (b.y - o.y) - (b.x - o.x) * (a.y - o.y); }

__host__ __device__ inline void rect_corners(const float *bx, P2 (&c)[5]) {
    const float hx = bx[3] / 2, hy = bx[4] / 2;
    const float ca = cosf(bx[6]), sa = sinf(bx[6]);
    const float lx[4] = {-hx, hx, hx, -hx}, ly[4] = {-hy, -hy, hy, hy};
    for (int k = 0; k < 4; ++k) {
        // rotate the axis-aligned corner about the centre
        const float px = bx[0] + lx[k], py = bx[1] + ly[k];
        c[k].x = (px - bx[0]) * ca + (py - bx[1]) * (-sa) + bx[0];
        c[k].y = (px - bx[0]) * sa + (py - bx[1]) * ca + bx[1];
    }
    c[4] = c[0];
}

__host__ __device__ inline bool inside_rect(const float *bx, const P2 &p) {
    const float margin = 1e-2f;
    const float ca = cosf(-bx[6]), sa = sinf(-bx[6]);
    const float rx = (p.x - bx[0]) * ca + (p.y - bx[1]) * (-sa);
    const float ry = (p.x - bx[0]) * sa + (p.y - bx[1]) * ca;
    return fabsf(rx) < bx[3] / 2 + margin && fabsf(ry) < bx[4] / 2 + margin;
}

// proper intersection of segment p0-p1 with q0-q1 (bounding-box reject, strict opposite-side test)
__host__ __device__ inline bool seg_intersect(const P2 &p1, const P2 &p0, const P2 &q1, const P2 &q0, P2 &out) {
    const bool boxes_touch = fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
                             fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y);
    if (!boxes_touch) return false;
    const float s1 = cross2(q0, p1, p0), s2 = cross2(p1, q1, p0), s3 = cross2(p0, q1, q0), s4 = cross2(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross2(q1, p1, p0);
    if (fabsf(s5 - s1) > 1e-8f) {
        out.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        out.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {   // nearly parallel: solve the two line equations
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float d = a0 * b1 - a1 * b0;
        out.x = (b0 * c1 - b1 * c0) / d;
        out.y = (a1 * c0 - a0 * c1) / d;
    }
    return true;
}

// `pts` holds the (at most 16) polygon points: anything indexable that yields P2 lvalues - a local array, or a view of per-lane LDS
// rows for a kernel that must stay out of scratch memory (roi_head.hip)
template <typename Points>
__host__ __device__ inline float bev_overlap_with(const float *a, const float *b, Points &&pts) {
    P2 ca[5], cb[5];
    rect_corners(a, ca);
    rect_corners(b, cb);
    int cnt = 0;
    float sx = 0.f, sy = 0.f;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            if (seg_intersect(ca[i + 1], ca[i], cb[j + 1], cb[j], pts[cnt])) {
                sx += pts[cnt].x; sy += pts[cnt].y;
                ++cnt;
            }
    for (int k = 0; k < 4; ++k) {
        if (inside_rect(a, cb[k])) { sx += cb[k].x; sy += cb[k].y; pts[cnt++] = cb[k]; }
        if (inside_rect(b, ca[k])) { sx += ca[k].x; sy += ca[k].y; pts[cnt++] = ca[k]; }
    }
    const P2 ctr{sx / cnt, sy / cnt};
    // order by angle around the centroid (exchange sort, as the reference: descending-angle pairs are swapped)
    for (int j = 0; j < cnt - 1; ++j)
        for (int i = 0; i < cnt - j - 1; ++i)
            if (atan2f(pts[i].y - ctr.y, pts[i].x - ctr.x) > atan2f(pts[i + 1].y - ctr.y, pts[i + 1].x - ctr.x)) {
                const P2 tmp = pts[i];
                pts[i] = pts[i + 1];
                pts[i + 1] = tmp;
            }
    float area = 0.f;
    for (int k = 0; k < cnt - 1; ++k)
        area += (pts[k].x - pts[0].x) * (pts[k + 1].y - pts[0].y) - (pts[k].y - pts[0].y) * (pts[k + 1].x - pts[0].x);
    return fabsf(area) / 2.0f;
}

__host__ __device__ inline float bev_overlap(const float *a, const float *b) {
    P2 pts[16];
    return bev_overlap_with(a, b, pts);
}

__host__ __device__ inline float bev_iou(const float *a, const float *b) {
    const float sa = a[3] * a[4], sb = b[3] * b[4];
    const float ov = bev_overlap(a, b);
    return ov / fmaxf(sa + sb - ov, 1e-8f);
}

}  // namespace s2d
