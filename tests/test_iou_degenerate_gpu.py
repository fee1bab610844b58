"""The device's rotated-box geometry (csrc/nms_geom.h behind nms.boxes_iou_bev, nms.rotate_nms, nms.rotate_nms_batched and the RoI
matcher second_stage.match_rois_to_gt) on the degenerate families of tests/golden/iou_pairs.npz, against what the REFERENCE's own CPU
implementation returned for them (tests/golden/make_golden_iou.py; tests/test_iou_pin.py holds the C oracle to the same numbers).

Tolerance of a value: 1e-5 + 4 sens.  1e-5 is the suite's device-vs-oracle bound (tests/test_nms.py); `sens` is how far the reference's
own result moves when one input moves by one float32 ulp, and the factor 4 lets the device's sinf / cosf of both boxes differ from the
host's by up to two ulps each.  Pairs the reference itself cannot hold still (`ill`: sens > 1e-3 or a NaN) are not compared."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 32
FAMILIES = ["identical", "yaw_pi", "swap_dims", "heading_eps", "centre_eps", "slide", "share_edge", "contained", "corner", "axis_aligned",
            "pedestrian", "generic"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "iou_pairs.npz")))


def _tol(sens):
    return 1e-5 + 4 * sens.astype(np.float64)


def _greedy(iou, thr):
    """the reference's greedy walk: rows in descending-score order, row i suppresses a later row j when iou[i, j] > thr"""
    alive, keep = np.ones(len(iou), bool), []
    for i in range(len(iou)):
        if alive[i]:
            keep.append(i)
            alive[i + 1:] &= ~(iou[i, i + 1:] > thr)
    return keep


# ---- IoU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_device_iou_matches_the_reference_binary(gold, family):
    """the whole 2K x 2K matrix of the family: its A x B block is `iou_ref`, the other blocks add the generic pairs and every box with itself"""
    from sparse2dense_amd import nms
    p = torch.from_numpy(gold[f"{family}/P"]).cuda()
    got = nms.boxes_iou_bev(p, p).cpu().numpy()
    want, sens, ill, nan = (gold[f"{family}/{k}_full"] for k in ("iou", "sens", "ill", "nan"))
    assert np.array_equal(gold[f"{family}/iou_ref"], want[:K, K:])
    diff = np.abs(got.astype(np.float64) - want)
    excess = np.where(ill, -np.inf, diff - _tol(sens))
    blk = diff[:K, K:][~ill[:K, K:]]
    print(f"{family}: max |device - reference| A x B {blk.max():.3e} (diagonal {np.diag(diff[:K, K:])[~np.diag(ill[:K, K:])].max():.3e}), "
          f"all 2K x 2K {diff[~ill].max():.3e}; largest sens {sens[~ill].max():.3e}; ill pairs {int(ill.sum())}")
    for i, j in np.argwhere(ill):
        print(f"  ill pair ({i}, {j}): reference {want[i, j]!r} (sens {sens[i, j]:.3g}, NaN seen {bool(nan[i, j])}), device {got[i, j]!r}")
    assert not np.isnan(got[~nan]).any(), np.argwhere(np.isnan(got) & ~nan).tolist()
    bad = np.argwhere(excess > 0)
    assert len(bad) == 0, [(int(i), int(j), float(got[i, j]), float(want[i, j]), float(sens[i, j])) for i, j in bad[:8]]


# ---- NMS ----------------------------------------------------------------------------------------------------------------------------------
def _segments(gold, which):
    """[(name, pcdet rows in descending-score order, reference IoU matrix of those rows)] and the two thresholds per segment"""
    segs = []
    for f in FAMILIES:
        order = gold[f"{f}/nms_order"]
        segs.append((f, gold[f"{f}/P"][order], gold[f"{f}/iou_full"][np.ix_(order, order)], float(gold[f"{f}/nms_thr"][which])))
    return segs


@pytest.mark.parametrize("which", [0, 1])
def test_rotate_nms_keeps_what_the_greedy_walk_over_the_reference_keeps(gold, which):
    from sparse2dense_amd import nms
    for name, rows, iou, thr in _segments(gold, which):
        scores = -torch.arange(len(rows), dtype=torch.float32)
        sel = nms.rotate_nms(torch.from_numpy(rows).cuda(), scores.cuda(), thr).cpu().tolist()
        assert sel == _greedy(iou, np.float32(thr)), (name, thr)
    dup = torch.from_numpy(gold["dup40/P"]).cuda()
    assert float(gold["dup40/iou_self"][0, 0]) > 0.9
    assert nms.rotate_nms(dup, torch.zeros(40).cuda(), thr).cpu().tolist() == [0]   # a stable sort: the first of equal scores
    rot = gold["rot8/P"]
    sel = nms.rotate_nms(torch.from_numpy(rot).cuda(), -torch.arange(8, dtype=torch.float32).cuda(), thr).cpu().tolist()
    assert sel == _greedy(gold["rot8/iou_full"], np.float32(thr)) == [0]


def test_rotate_nms_batched_over_all_families_as_segments_of_one_call(gold):
    """every family, the 40 identical boxes and the rectangle written eight ways are the segments of each call.  The entry takes one
    threshold per call and the fixture holds one per family (near 0.1, near 0.7): one call per distinct value, in which the segments
    that own the value, and the two extra segments, are checked"""
    from sparse2dense_amd import nms
    for which in (0, 1):
        segs = _segments(gold, which)
        segs.append(("dup40", gold["dup40/P"], np.full((40, 40), gold["dup40/iou_self"][0, 0], np.float32), None))
        segs.append(("rot8", gold["rot8/P"], gold["rot8/iou_full"], None))
        counts = [len(s[1]) for s in segs]
        offsets = np.concatenate([[0], np.cumsum(counts)[:-1]])
        packed = torch.from_numpy(np.concatenate([s[1] for s in segs])).cuda()
        seg = torch.from_numpy(np.stack([offsets, counts]).astype(np.int32)).cuda()
        checked = 0
        for thr in sorted({s[3] for s in segs if s[3] is not None}):
            keep, n_keep = nms.rotate_nms_batched(packed, seg, counts, thr)
            assert keep.shape == (len(segs), max(counts))
            for s, (name, rows, iou, own) in enumerate(segs):
                if own is None or own == thr:
                    assert keep[s, :n_keep[s]].cpu().tolist() == _greedy(iou, np.float32(thr)), (name, thr)
                    checked += 1
                if name in ("dup40", "rot8"):
                    assert n_keep[s] == 1, (name, thr)
        assert checked >= len(FAMILIES) + 2


# ---- the RoI matcher ----------------------------------------------------------------------------------------------------------------------
N_ROI, N_GT = 33, 70
LAYOUTS = {"equal": 0.0, "half": 1.0, "touching": 2.0}   # z of the structured ground truth; RoIs have z = 0, every height is 2


def _match_case(gold, family, layout):
    """rois [2, 33, 7], labels [2, 33], gt [2, 70, 8] (det3d rows + class) and, per sample, the row of `P` behind every RoI / gt row.
    Sample 0: RoIs = A and one B box; gt = B (classes 1, 2 alternating), rows 32..37 bit-identical copies of B rows 0..5, rows 38..69 the
    A boxes as class 3 - the first 16 exactly touching the RoIs from above (oh == 0), the others 0.5 m up.  Sample 1: the RoIs reversed
    and the gt rows permuted, which moves structured rows behind row 63 and some copies in front of their originals."""
    d = gold[f"{family}/D"]
    roi_c = np.concatenate([np.arange(K), [K]])
    gt_c = np.concatenate([K + np.arange(K), K + np.arange(6), np.arange(K)])
    gt_cls = np.concatenate([1 + np.arange(K) % 2, 1 + np.arange(6) % 2, np.full(K, 3)])
    gt_z = np.concatenate([np.full(K + 6, LAYOUTS[layout]), np.full(16, 2.0), np.full(16, 0.5)])
    roi_lab = np.concatenate([1 + np.arange(K) % 2, [3]])
    perm = np.random.RandomState(5).permutation(N_GT)
    samples = [(roi_c, roi_lab, gt_c, gt_cls, gt_z), (roi_c[::-1].copy(), roi_lab[::-1].copy(), gt_c[perm], gt_cls[perm], gt_z[perm])]
    rois, labels, gt = np.zeros((2, N_ROI, 7), np.float32), np.zeros((2, N_ROI), np.int64), np.zeros((2, N_GT, 8), np.float32)
    for b, (rc, rl, gc, gcl, gz) in enumerate(samples):
        rois[b], labels[b] = d[rc], rl
        rois[b, :, 2], rois[b, :, 5] = 0.0, 2.0
        gt[b, :, :7], gt[b, :, 7] = d[gc], gcl
        gt[b, :, 2], gt[b, :, 5] = gz, 2.0
    return rois, labels, gt, samples


def _expected_iou3d(gold, family, rc, gc, gz):
    """float64 3-D IoU [33, 70] from the reference's BEV IoU: ov = iou (sa + sb) / (1 + iou), then ov oh / max(va + vb - ov oh, 1e-6)"""
    p = gold[f"{family}/P"].astype(np.float64)
    iou = gold[f"{family}/iou_full"][np.ix_(rc, gc)].astype(np.float64)
    sa, sb = (p[rc, 3] * p[rc, 4])[:, None], (p[gc, 3] * p[gc, 4])[None, :]
    ov = iou * (sa + sb) / (1 + iou)
    oh = np.maximum(np.minimum(1.0, gz + 1.0) - np.maximum(-1.0, gz - 1.0), 0.0)[None, :]
    return ov * oh / np.maximum(sa * 2.0 + sb * 2.0 - ov * oh, 1e-6), oh


@pytest.mark.parametrize("family", FAMILIES)
def test_roi_matcher_on_degenerate_pairs(gold, family):
    from sparse2dense_amd import second_stage as S
    worst, skipped = 0.0, 0
    for layout in LAYOUTS:
        rois, labels, gt, samples = _match_case(gold, family, layout)
        for by_class in (True, False):
            got_iou, got_arg, count = [t.cpu().numpy() for t in S.match_rois_to_gt(torch.from_numpy(rois).cuda(), torch.from_numpy(labels).cuda(),
                                                                                  torch.from_numpy(gt).cuda(), by_class=by_class)]
            assert count.tolist() == [N_GT, N_GT] and got_iou.shape == got_arg.shape == (2, N_ROI)
            for b, (rc, rl, gc, gcl, gz) in enumerate(samples):
                want, oh = _expected_iou3d(gold, family, rc, gc, gz)
                tol = _tol(gold[f"{family}/sens_full"][np.ix_(rc, gc)])
                ill = gold[f"{family}/ill_full"][np.ix_(rc, gc)] & (oh > 0)      # with oh == 0 the BEV value does not matter
                nan = gold[f"{family}/nan_full"][np.ix_(rc, gc)] & (oh > 0)
                for i in range(N_ROI):
                    cand = (gcl == rl[i]) if by_class else np.ones(N_GT, bool)
                    assert cand.any()
                    where = (family, layout, by_class, b, i)
                    arg, val = int(got_arg[b, i]), float(got_iou[b, i])
                    assert cand[arg], where
                    if not nan[i, cand].any():
                        assert not np.isnan(val), where
                    if ill[i, cand].any():
                        skipped += 1
                        print(f"  {where}: an ill pair among the candidates, device max_iou {val!r} row {arg}")
                        continue
                    m = want[i, cand].max()
                    near = cand & (want[i] >= m - 2 * tol[i])            # the rows that may hold the device's maximum
                    t = tol[i, near].max()
                    worst = max(worst, abs(val - m))
                    assert abs(val - m) <= t, where + (val, m, t)
                    assert near[arg], where + (arg, float(want[i, arg]), m)
                    # bit-identical ground-truth rows: the lowest row wins
                    same = np.flatnonzero(cand & (gt[b].view(np.uint32) == gt[b, arg].view(np.uint32)).all(1))
                    assert arg == same[0], where + (arg, same.tolist())
                    if (oh[0, cand] == 0).all():                          # heights exactly touching: IoU exactly 0, the first candidate row
                        assert val == 0.0 and arg == np.flatnonzero(cand)[0], where + (val, arg)
                    if family == "corner" and m > 0:                      # the pre-clip reject must not drop a pair the reference counts
                        assert val != 0.0, where + (m,)
    print(f"{family}: max |device max_iou - expected| {worst:.3e}; RoIs left out for an ill candidate pair: {skipped}")
