#!/usr/bin/env python
"""Generates the rotated-IoU pin fixture by RUNNING the reference's own CPU implementation (det3d/ops/iou3d_nms/src/iou3d_cpu.cpp,
compiled read-only by oracle/ref_iou3d.py into oracle/_ref/) in the build container:

    python tests/golden/make_golden_iou.py

  iou_pairs.npz   for each family of FAMILIES: K = 32 boxes A and K boxes B, pair (i, i) the structured case, all 2K boxes inside one
                  patch so that the other pairs overlap generically.  `<f>/D` [2K, 7] the boxes in det3d convention (x, y, z, w, l, h,
                  yaw; rows 0..K-1 = A, K..2K-1 = B), `<f>/P` the pcdet rows the geometry sees (float32: dims swapped,
                  -yaw - float32(pi/2)).  Of the reference binary on P x P, [2K, 2K]: `<f>/iou_full`; `<f>/sens_full`, the largest
                  change of its OWN result when one of x, y, dx, dy, heading of either box moves by one float32 ulp in either
                  direction (20 matrix calls); `<f>/nan_full`, a NaN among those 21 values; `<f>/ill_full` = sens > 1e-3 or NaN.
                  The A x B blocks again as `<f>/iou_ref`, `<f>/sens`, `<f>/ill`, `<f>/ref_nan` [K, K], and `<f>/iou_exact`: the
                  float64 Sutherland-Hodgman clip of the same float32 rows (informational).
                  NMS: `<f>/nms_order`, the rows of P that take part (no box of an ill pair) in descending-score order, and
                  `<f>/nms_thr` (two float32 thresholds near 0.1 and 0.7, moved until every reference IoU among those rows keeps
                  1e-3 + 4 sens away).  `dup40/P`: one box 40 times; `rot8/P`, `rot8/iou_full`: one rectangle written with
                  yaw + k pi/2 and the dims swapped for odd k.

Only boxes (generated here) and what the reference binary returned for them are stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_iou3d  # noqa: E402

K = 32
SEED = 20260
FAMILIES = ["identical", "yaw_pi", "swap_dims", "heading_eps", "centre_eps", "slide", "share_edge", "contained", "corner", "axis_aligned",
            "pedestrian", "generic"]
ILL_SENS = 1e-3
ILL_CAP_TOTAL, ILL_CAP_DIAG = 0.005, 2
PI = np.pi


# ---- boxes --------------------------------------------------------------------------------------------------------------------------------
def _det3d(cx, cy, length, width, theta, rs):
    """float32 det3d rows of rectangles given by centre, length, width and the direction `theta` of the length axis (the pcdet heading)"""
    n = len(cx)
    d = np.zeros((n, 7), np.float64)
    d[:, 0], d[:, 1], d[:, 2] = cx, cy, rs.uniform(-1, 1, n)
    d[:, 3], d[:, 4], d[:, 5] = width, length, rs.uniform(1, 2, n)
    d[:, 6] = -np.asarray(theta) - PI / 2
    return d.astype(np.float32)


def to_pcdet(d):
    """the two operations of the device's to_pcdet, in float32"""
    p = d[:, [0, 1, 2, 4, 3, 5, 6]].astype(np.float32)
    p[:, 6] = -d[:, 6] - np.float32(1.5707964)
    assert p.dtype == np.float32
    return p


def _base(rs, patch=30.0, centre_max=45.0, lrange=(0.3, 12.0), wrange=(0.3, 3.0)):
    c0 = rs.uniform(-centre_max, centre_max, 2)
    half = patch / 2 - 1.0
    cx, cy = c0[0] + rs.uniform(-half, half, K), c0[1] + rs.uniform(-half, half, K)
    return cx, cy, rs.uniform(*lrange, K), rs.uniform(*wrange, K), rs.uniform(-PI, PI, K)


def _along(theta):
    return np.cos(theta), np.sin(theta)


def family_boxes(name, rs):
    cx, cy, ln, wd, th = _base(rs)
    ux, uy = _along(th)            # the length axis
    vx, vy = -uy, ux               # the width axis
    if name in ("identical", "yaw_pi", "swap_dims", "heading_eps", "centre_eps"):
        a = _det3d(cx, cy, ln, wd, th, rs)
        b = a.copy()
        if name == "yaw_pi":
            b[:, 6] = (a[:, 6].astype(np.float64) + PI).astype(np.float32)
        elif name == "swap_dims":
            b[:, 3], b[:, 4] = a[:, 4], a[:, 3]
            b[:, 6] = (a[:, 6].astype(np.float64) + PI / 2).astype(np.float32)
        elif name == "heading_eps":
            b[:, 6] = (a[:, 6].astype(np.float64) + rs.uniform(-1e-3, 1e-3, K)).astype(np.float32)
        elif name == "centre_eps":
            b[:, :2] = (a[:, :2].astype(np.float64) + rs.uniform(-1e-3, 1e-3, (K, 2))).astype(np.float32)
        return a, b
    if name == "slide":            # same width and heading, another length, moved along the heading: collinear long edges
        lb = rs.uniform(0.3, 12.0, K)
        s = rs.uniform(-0.9, 0.9, K) * (ln + lb) / 2
        return _det3d(cx, cy, ln, wd, th, rs), _det3d(cx + s * ux, cy + s * uy, lb, wd, th, rs)
    if name == "share_edge":       # side by side on a long edge: the first half fully, the second half partially
        wb = rs.uniform(0.3, 3.0, K)
        s = np.where(np.arange(K) < K // 2, 0.0, rs.uniform(0.2, 0.8, K) * ln)
        off = (wd + wb) / 2
        return _det3d(cx, cy, ln, wd, th, rs), _det3d(cx + s * ux + off * vx, cy + s * uy + off * vy, ln, wb, th, rs)
    if name == "contained":        # B inside A: the first half with A's heading, the second half rotated
        ln, wd = rs.uniform(2.0, 12.0, K), rs.uniform(1.5, 3.0, K)
        lb = np.where(np.arange(K) < K // 2, rs.uniform(0.2, 0.6, K) * ln, rs.uniform(0.3, 0.55, K) * wd)
        wb = rs.uniform(0.3, 0.55, K) * wd
        tb = np.where(np.arange(K) < K // 2, th, rs.uniform(-PI, PI, K))
        o = rs.uniform(-0.05, 0.05, (2, K)) * wd
        return _det3d(cx, cy, ln, wd, th, rs), _det3d(cx + o[0], cy + o[1], lb, wb, tb, rs)
    if name == "corner":           # a corner of B at a corner of A, the gap along A's diagonal in [-0.02, +0.02] m: around the 1e-2 margin
        gap = rs.uniform(-0.02, 0.02, K)
        first = np.arange(K) < K // 2
        scale = rs.uniform(0.5, 1.5, K)                      # first half: B is A scaled - the centres are the two half diagonals + gap apart
        lb = np.where(first, np.clip(ln * scale, 0.3, 12.0), rs.uniform(0.3, 12.0, K))
        wb = np.where(first, np.clip(wd * scale, 0.3, 3.0), rs.uniform(0.3, 3.0, K))
        phi = np.where(first, 0.0, rs.uniform(-PI / 2, PI / 2, K))   # second half: B turned about the shared corner, still outside A
        g = gap / np.sqrt(2.0)
        kx, ky = cx + (ln / 2 + g) * ux + (wd / 2 + g) * vx, cy + (ln / 2 + g) * uy + (wd / 2 + g) * vy   # B's (-l/2, -w/2) corner
        bux, buy = _along(th + phi)
        bcx, bcy = kx + lb / 2 * bux + wb / 2 * -buy, ky + lb / 2 * buy + wb / 2 * bux
        return _det3d(cx, cy, ln, wd, th, rs), _det3d(bcx, bcy, lb, wb, th + phi, rs)
    if name == "axis_aligned":     # headings are multiples of pi / 2
        th = rs.randint(-2, 3, K) * (PI / 2)
        tb = rs.randint(-2, 3, K) * (PI / 2)
        lb, wb = rs.uniform(0.3, 12.0, K), rs.uniform(0.3, 3.0, K)
        o = rs.uniform(-1, 1, (2, K))
        return _det3d(cx, cy, ln, wd, th, rs), _det3d(cx + o[0] * ln / 2, cy + o[1] * wd / 2, lb, wb, tb, rs)
    if name == "pedestrian":       # 0.3 - 0.8 m boxes far from the origin: a 6 m cluster whose coordinates reach |x|, |y| = 150 m
        sx, sy = rs.choice([-1.0, 1.0], 2)
        cx, cy = sx * (147.0 + rs.uniform(-3, 3, K)), sy * (147.0 + rs.uniform(-3, 3, K))
        ln, wd, lb, wb = (rs.uniform(0.3, 0.8, K) for _ in range(4))
        o = rs.uniform(-0.3, 0.3, (2, K))
        bx, by = np.clip(cx + o[0], -150, 150), np.clip(cy + o[1], -150, 150)
        return _det3d(cx, cy, ln, wd, th, rs), _det3d(bx, by, lb, wb, rs.uniform(-PI, PI, K), rs)
    if name == "generic":
        o = rs.uniform(-2, 2, (2, K))
        return _det3d(cx, cy, ln, wd, th, rs), _det3d(cx + o[0], cy + o[1], rs.uniform(0.3, 12.0, K), rs.uniform(0.3, 3.0, K),
                                                       rs.uniform(-PI, PI, K), rs)
    raise KeyError(name)


# ---- the float64 clip (as tests/test_nms.py) ----------------------------------------------------------------------------------------------
def _poly(b):
    x, y, dx, dy, a = (float(v) for v in (b[0], b[1], b[3] / 2, b[4] / 2, b[6]))
    c, s = np.cos(a), np.sin(a)
    pts = np.array([[-dx, -dy], [dx, -dy], [dx, dy], [-dx, dy]], np.float64)
    return pts @ np.array([[c, s], [-s, c]]) + [x, y]


def _clip_area(p, q):
    out = [tuple(v) for v in p]
    for i in range(len(q)):
        a, b = q[i], q[(i + 1) % len(q)]
        inp, out = out, []
        if not inp:
            break
        side = lambda v: (b[0] - a[0]) * (v[1] - a[1]) - (b[1] - a[1]) * (v[0] - a[0])  # noqa: E731
        for j in range(len(inp)):
            cur, nxt = inp[j], inp[(j + 1) % len(inp)]
            sc, sn = side(cur), side(nxt)
            if sc >= 0:
                out.append(cur)
            if (sc >= 0) != (sn >= 0):
                t = sc / (sc - sn)
                out.append((cur[0] + t * (nxt[0] - cur[0]), cur[1] + t * (nxt[1] - cur[1])))
    if len(out) < 3:
        return 0.0
    o = np.array(out)
    return 0.5 * abs(np.dot(o[:, 0], np.roll(o[:, 1], -1)) - np.dot(o[:, 1], np.roll(o[:, 0], -1)))


def exact_iou(pa, pb):
    polys_a, polys_b = [_poly(b) for b in pa], [_poly(b) for b in pb]
    out = np.zeros((len(pa), len(pb)), np.float64)
    for i, a in enumerate(pa):
        for j, b in enumerate(pb):
            inter = _clip_area(polys_a[i], polys_b[j])
            out[i, j] = inter / max(float(a[3]) * float(a[4]) + float(b[3]) * float(b[4]) - inter, 1e-8)
    return out


# ---- the reference binary -----------------------------------------------------------------------------------------------------------------
def reference_and_sensitivity(p):
    """(iou, sens, nan) of the reference binary on p x p: see the module docstring"""
    base = ref_iou3d.boxes_iou_bev(p, p)
    sens = np.zeros_like(base)
    nan = np.isnan(base)
    for col in (0, 1, 3, 4, 6):
        for toward in (np.float32(-np.inf), np.float32(np.inf)):
            q = p.copy()
            q[:, col] = np.nextafter(p[:, col], toward)
            for moved in (ref_iou3d.boxes_iou_bev(q, p), ref_iou3d.boxes_iou_bev(p, q)):
                nan |= np.isnan(moved)
                with np.errstate(invalid="ignore"):
                    sens = np.fmax(sens, np.abs(moved - base))
    return base, sens, nan


def greedy(iou, thr):
    """the greedy loop over an IoU matrix whose rows are in descending-score order (row i suppresses a later j when iou[i, j] > thr)"""
    alive, keep = np.ones(len(iou), bool), []
    for i in range(len(iou)):
        if alive[i]:
            keep.append(i)
            alive[i + 1:] &= ~(iou[i, i + 1:] > thr)
    return keep


def clear_threshold(matrices, start):
    """the float32 threshold nearest `start` from which every off-diagonal entry of every (iou, sens) keeps more than 1e-3 + 4 sens"""
    v = np.concatenate([iou[~np.eye(len(iou), dtype=bool)].astype(np.float64) for iou, _ in matrices])
    s = np.concatenate([sens[~np.eye(len(sens), dtype=bool)].astype(np.float64) for _, sens in matrices])
    for k in range(400):
        for sign in (1, -1):
            t = np.float32(start + sign * k * 5e-4)
            if np.all(np.abs(v - float(t)) > 1e-3 + 4 * s):
                return t
    raise AssertionError(f"no clear threshold near {start}")


def main():
    assert ref_iou3d.reference_present(), "the reference tree is needed to generate this fixture"
    ref_iou3d.build()
    rs = np.random.RandomState(SEED)
    out, ill_total, report, nms_sets = {}, 0, [], []
    for name in FAMILIES:
        a, b = family_boxes(name, rs)
        d = np.concatenate([a, b])
        p = to_pcdet(d)
        iou, sens, nan = reference_and_sensitivity(p)
        ill = (sens > ILL_SENS) | nan
        exact = exact_iou(p[:K], p[K:])
        blk = (slice(0, K), slice(K, 2 * K))
        n_ill, n_diag = int(ill[blk].sum()), int(np.diag(ill[blk]).sum())
        assert n_diag <= ILL_CAP_DIAG, (name, n_diag)
        ill_total += n_ill
        # NMS: no box of an ill pair (the box with itself is not a pair of the NMS)
        off = ill & ~np.eye(2 * K, dtype=bool)
        bad = off.any(0) | off.any(1)
        rows = np.flatnonzero(~bad)
        order = rows[rs.permutation(len(rows))]
        sub, ssub = iou[np.ix_(order, order)], sens[np.ix_(order, order)]
        nms_sets.append((name, sub, ssub))
        good = ~ill[blk]
        report.append(f"{name:13s} ill {n_ill:3d} (diagonal {n_diag}), full-matrix ill {int(ill.sum()):3d}, pairs with IoU > 0: "
                      f"{int((iou[blk] > 0).sum()):4d}, max |ref - exact| {np.abs(iou[blk] - exact)[good].max():.4f}, "
                      f"diag IoU {np.diag(iou[blk]).min():.4f}..{np.diag(iou[blk]).max():.4f}, NMS rows {len(order)}")
        for key, val in dict(D=d, P=p, iou_full=iou, sens_full=sens, nan_full=nan, ill_full=ill, iou_ref=iou[blk], sens=sens[blk],
                             ill=ill[blk], ref_nan=nan[blk], iou_exact=exact, nms_order=order.astype(np.int64)).items():
            out[f"{name}/{key}"] = np.ascontiguousarray(val)
    assert ill_total <= ILL_CAP_TOTAL * len(FAMILIES) * K * K, ill_total
    # one box 40 times, and one rectangle written eight ways
    a, _ = family_boxes("generic", rs)
    for i in range(K):
        one = a[i:i + 1]
        rot = np.repeat(one, 8, 0)
        for k in range(8):
            rot[k, 6] = np.float32(float(one[0, 6]) + k * PI / 2)
            if k % 2:
                rot[k, 3], rot[k, 4] = one[0, 4], one[0, 3]
        p = to_pcdet(rot)
        iou, sens, nan = reference_and_sensitivity(p)
        off = ~np.eye(8, dtype=bool)
        if not nan.any() and sens.max() <= ILL_SENS and np.all(iou[off] > 0.9):
            break
    else:
        raise AssertionError("no well-conditioned box for the rot8 segment")
    out["rot8/P"], out["rot8/iou_full"] = p, iou
    # per family the thresholds nearest 0.1 and 0.7 that are clear of every IoU that takes part (rot8 / dup40: all IoUs above 0.9)
    for name, sub, ssub in nms_sets:
        thr = np.array([clear_threshold([(sub, ssub)], 0.1), clear_threshold([(sub, ssub)], 0.7)], np.float32)
        out[f"{name}/nms_thr"] = thr
        report.append(f"{name:13s} NMS thresholds {thr} keep {[len(greedy(sub, t)) for t in thr]} of {len(sub)}")
    dup = np.repeat(to_pcdet(one), 40, 0)
    self_iou = ref_iou3d.boxes_iou_bev(dup[:1], dup[:1])
    assert self_iou[0, 0] > 0.9
    out["dup40/P"], out["dup40/iou_self"] = dup, self_iou
    out["seed"] = np.int64(SEED)
    path = os.path.join(HERE, "iou_pairs.npz")
    np.savez_compressed(path, **out)
    print("\n".join(report))
    print(f"ill pairs in all A x B blocks: {ill_total} of {len(FAMILIES) * K * K}")
    print(f"wrote iou_pairs.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
