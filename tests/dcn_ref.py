"""Float64 numpy restatement of deformable convolution v1, written from its semantics with explicit loops - deliberately a different
formulation from sparse2dense_amd.dcn.deform_conv_composite (which gathers whole tensors and lets autograd differentiate):

  position   h = ho*stride - pad + i*dil + off_h,  w alike; offset channel g*2*K + 2*(i*kw+j) is the row offset, + 1 the column offset
  value      0 unless h > -1 and w > -1 and h < H and w < W (strict); else the bilinear blend over floor(h), floor(h)+1 x floor(w), floor(w)+1,
             each corner contributing only inside [0, H-1] x [0, W-1]
  backward   the analytic formulas of the reference's get_gradient_weight (input) and get_coordinate_weight (offset; floor as in the forward,
             i.e. the right-hand derivative at integer positions), not autograd
"""
import math

import numpy as np


def _out(h, k, s, p, d):
    return (h + 2 * p - (d * (k - 1) + 1)) // s + 1


def sample(img, h, w):
    """img [H, W] -> masked bilinear value at (h, w)"""
    H, W = img.shape
    if not (h > -1 and w > -1 and h < H and w < W):
        return 0.0
    hl, wl = math.floor(h), math.floor(w)
    lh, lw = h - hl, w - wl
    v = 0.0
    if hl >= 0 and wl >= 0:
        v += (1 - lh) * (1 - lw) * img[hl, wl]
    if hl >= 0 and wl + 1 <= W - 1:
        v += (1 - lh) * lw * img[hl, wl + 1]
    if hl + 1 <= H - 1 and wl >= 0:
        v += lh * (1 - lw) * img[hl + 1, wl]
    if hl + 1 <= H - 1 and wl + 1 <= W - 1:
        v += lh * lw * img[hl + 1, wl + 1]
    return v


def _positions(offset, n, g, tap, kw, ho, wo, stride, pad, dil, K):
    i, j = divmod(tap, kw)
    h = ho * stride - pad + i * dil + offset[n, g * 2 * K + 2 * tap, ho, wo]
    w = wo * stride - pad + j * dil + offset[n, g * 2 * K + 2 * tap + 1, ho, wo]
    return h, w


def forward(x, offset, weight, stride=1, pad=0, dil=1, groups=1, dg=1):
    x, offset, weight = (np.asarray(a, dtype=np.float64) for a in (x, offset, weight))
    N, C, H, W = x.shape
    Cout, Cg, kh, kw = weight.shape
    K = kh * kw
    Ho, Wo = _out(H, kh, stride, pad, dil), _out(W, kw, stride, pad, dil)
    cg, og = C // dg, Cout // groups
    y = np.zeros((N, Cout, Ho, Wo))
    for n in range(N):
        for ho in range(Ho):
            for wo in range(Wo):
                for tap in range(K):
                    for c in range(C):
                        h, w = _positions(offset, n, c // cg, tap, kw, ho, wo, stride, pad, dil, K)
                        v = sample(x[n, c], h, w)
                        if v == 0.0:
                            continue
                        grp = c // Cg
                        y[n, grp * og:(grp + 1) * og, ho, wo] += weight[grp * og:(grp + 1) * og, c - grp * Cg, tap // kw, tap % kw] * v
    return y


def backward(x, offset, weight, dy, stride=1, pad=0, dil=1, groups=1, dg=1):
    """-> dx, d_offset, dweight"""
    x, offset, weight, dy = (np.asarray(a, dtype=np.float64) for a in (x, offset, weight, dy))
    N, C, H, W = x.shape
    Cout, Cg, kh, kw = weight.shape
    K = kh * kw
    Ho, Wo = dy.shape[2:]
    cg, og = C // dg, Cout // groups
    dx, doff, dwt = np.zeros_like(x), np.zeros_like(offset), np.zeros_like(weight)
    for n in range(N):
        for ho in range(Ho):
            for wo in range(Wo):
                for tap in range(K):
                    i, j = divmod(tap, kw)
                    for c in range(C):
                        g, grp = c // cg, c // Cg
                        h, w = _positions(offset, n, g, tap, kw, ho, wo, stride, pad, dil, K)
                        d = dy[n, grp * og:(grp + 1) * og, ho, wo]
                        dwt[grp * og:(grp + 1) * og, c - grp * Cg, i, j] += d * sample(x[n, c], h, w)
                        dcol = float(np.dot(d, weight[grp * og:(grp + 1) * og, c - grp * Cg, i, j]))
                        if not (h > -1 and w > -1 and h < H and w < W):
                            continue
                        hl, wl = math.floor(h), math.floor(w)
                        lh, lw = h - hl, w - wl
                        img = x[n, c]
                        gh = gw = 0.0
                        for yy, xx, wgt, sh, sw in ((hl, wl, (1 - lh) * (1 - lw), -(1 - lw), -(1 - lh)),
                                                    (hl, wl + 1, (1 - lh) * lw, -lw, (1 - lh)),
                                                    (hl + 1, wl, lh * (1 - lw), (1 - lw), -lh),
                                                    (hl + 1, wl + 1, lh * lw, lw, lh)):
                            if 0 <= yy <= H - 1 and 0 <= xx <= W - 1:
                                dx[n, c, yy, xx] += wgt * dcol      # get_gradient_weight
                                gh += sh * img[yy, xx]              # get_coordinate_weight, bp_dir 0
                                gw += sw * img[yy, xx]              # bp_dir 1
                        doff[n, g * 2 * K + 2 * tap, ho, wo] += gh * dcol
                        doff[n, g * 2 * K + 2 * tap + 1, ho, wo] += gw * dcol
    return dx, doff, dwt
