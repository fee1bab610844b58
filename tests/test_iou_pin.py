"""The pin of the rotated-IoU oracle: oracle/iou_nms.c against what the REFERENCE's own CPU implementation (iou3d_cpu.cpp, built by
oracle/ref_iou3d.py) returned for the degenerate families of tests/golden/iou_pairs.npz (tests/golden/make_golden_iou.py): identical
boxes, heading + pi, swapped dims with heading + pi/2, millimetre duplicates, collinear and shared edges, containment, corner contacts
around the 1e-2 inside margin, axis-aligned headings, pedestrian-size boxes at 150 m and a generic control."""
import os
import sys

import numpy as np
import pytest

from oracle import iou_nms as O
from oracle import ref_iou3d

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_iou as G  # noqa: E402

K = G.K


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "iou_pairs.npz")))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_fixture_holds_every_family_in_both_conventions(gold):
    assert int(gold["seed"]) == G.SEED and len(G.FAMILIES) == 12
    for f in G.FAMILIES:
        d, p = gold[f"{f}/D"], gold[f"{f}/P"]
        assert d.shape == p.shape == (2 * K, 7) and d.dtype == p.dtype == np.float32
        assert np.array_equal(_bits(p), _bits(G.to_pcdet(d)))
        for key in ("iou_ref", "sens", "ill", "ref_nan", "iou_exact"):
            assert gold[f"{f}/{key}"].shape == (K, K), (f, key)
        assert np.array_equal(_bits(gold[f"{f}/iou_ref"]), _bits(gold[f"{f}/iou_full"][:K, K:]))
        assert np.array_equal(gold[f"{f}/ill"], (gold[f"{f}/sens"] > 1e-3) | gold[f"{f}/ref_nan"])
        assert np.array_equal(gold[f"{f}/ill_full"], (gold[f"{f}/sens_full"] > 1e-3) | gold[f"{f}/nan_full"])
    # the families are what they claim to be (det3d rows: x, y, z, w, l, h, yaw)
    a, b = gold["identical/D"][:K], gold["identical/D"][K:]
    assert np.array_equal(_bits(a), _bits(b))
    a, b = gold["swap_dims/D"][:K], gold["swap_dims/D"][K:]
    assert np.array_equal(a[:, 3], b[:, 4]) and np.array_equal(a[:, 4], b[:, 3]) and np.allclose(b[:, 6] - a[:, 6], np.pi / 2, atol=1e-6)
    a, b = gold["yaw_pi/D"][:K], gold["yaw_pi/D"][K:]
    assert np.array_equal(a[:, :6], b[:, :6]) and np.allclose(b[:, 6] - a[:, 6], np.pi, atol=1e-6)
    d = gold["pedestrian/D"]
    assert d[:, 3:5].max() <= 0.8 and d[:, 3:5].min() >= 0.3 and 149 < np.abs(d[:, :2]).max() <= 150
    h = gold["axis_aligned/P"][:, 6].astype(np.float64) / (np.pi / 2)
    assert np.abs(h - np.round(h)).max() < 1e-6
    for f in G.FAMILIES:
        if f != "pedestrian":
            d = gold[f"{f}/D"]
            assert np.abs(d[:, :2]).max() <= 75 and np.ptp(d[:K, 0]) <= 30 and np.ptp(d[:K, 1]) <= 30, f
    assert np.unique(gold["dup40/P"], axis=0).shape == (1, 7) and gold["dup40/P"].shape == (40, 7)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_oracle_is_bit_equal_to_the_reference_binary(gold, family):
    """(a) oracle/iou_nms.c == iou3d_cpu.cpp, bit for bit, on the whole 2K x 2K matrix of the family (the A x B block is `iou_ref`)"""
    p = gold[f"{family}/P"]
    got, want = O.bev_iou(p, p), gold[f"{family}/iou_full"]
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (family, np.argwhere(~same)[:8].tolist(), got[~same][:8], want[~same][:8])
    assert np.array_equal(_bits(O.bev_iou(p[:K], p[K:])), _bits(gold[f"{family}/iou_ref"])) or np.isnan(want[:K, K:]).any()


def test_oracle_is_bit_equal_on_the_extra_nms_segments(gold):
    p = gold["rot8/P"]
    assert np.array_equal(_bits(O.bev_iou(p, p)), _bits(gold["rot8/iou_full"]))
    d = gold["dup40/P"]
    assert np.array_equal(_bits(O.bev_iou(d[:1], d[:1])), _bits(gold["dup40/iou_self"]))


@pytest.mark.parametrize("family", G.FAMILIES)
def test_reference_agrees_with_the_exact_clip_outside_ill_pairs(gold, family):
    """(b) |iou_ref - iou_exact| <= 3e-2 outside `ill`: the reference counts a corner within 1e-2 m of a box as inside it, which on
    boxes as small as 0.3 m is a band of a few per cent of the area.  Largest value in the committed fixture: 1.78e-2 (heading_eps;
    pedestrian 1.39e-2, centre_eps 8.5e-3, every other family below 6e-4)."""
    good = ~gold[f"{family}/ill"]
    diff = np.abs(gold[f"{family}/iou_ref"].astype(np.float64) - gold[f"{family}/iou_exact"])[good]
    print(f"{family}: max |iou_ref - iou_exact| = {diff.max():.3e}")
    assert diff.max() <= 3e-2, (family, diff.max())
    # and the stored clip is the clip of the stored boxes (spot check: the diagonal and one row)
    p = gold[f"{family}/P"]
    again = G.exact_iou(p[:K], p[K:K + 1])[:, 0]
    assert np.array_equal(again, gold[f"{family}/iou_exact"][:, 0])


def test_ill_conditioned_pairs_stay_within_the_caps(gold):
    """(d) at most 0.5 % of all A x B pairs, and at most 2 per family diagonal, are ill-conditioned for the reference itself"""
    total = 0
    for f in G.FAMILIES:
        ill = gold[f"{f}/ill"]
        total += int(ill.sum())
        print(f"{f}: {int(ill.sum())} ill pairs, {int(np.diag(ill).sum())} on the diagonal")
        assert int(np.diag(ill).sum()) <= 2, f
    assert total <= 0.005 * len(G.FAMILIES) * K * K, total


@pytest.mark.parametrize("family", G.FAMILIES)
def test_nms_thresholds_are_clear_of_every_reference_iou(gold, family):
    iou, sens, order = gold[f"{family}/iou_full"], gold[f"{family}/sens_full"], gold[f"{family}/nms_order"]
    off = gold[f"{family}/ill_full"] & ~np.eye(2 * K, dtype=bool)
    assert not off[np.ix_(order, order)].any() and len(set(order.tolist())) == len(order) >= K
    sub, ssub = iou[np.ix_(order, order)].astype(np.float64), sens[np.ix_(order, order)].astype(np.float64)
    thr = gold[f"{family}/nms_thr"]
    assert thr.dtype == np.float32 and abs(thr[0] - 0.1) < 0.05 and abs(thr[1] - 0.7) < 0.05
    pairs = ~np.eye(len(order), dtype=bool)
    for t in thr:
        assert np.all(np.abs(sub - float(t))[pairs] > 1e-3 + 4 * ssub[pairs]), (family, t)
        # the C oracle's own greedy NMS walks the same matrix
        p = gold[f"{family}/P"][order]
        got = O.rotate_nms(p, -np.arange(len(p), dtype=np.float32), float(t)).tolist()
        assert got == G.greedy(iou[np.ix_(order, order)], t), (family, t)


def test_regenerating_from_the_reference_binary_reproduces_the_fixture(gold):
    """(c) needs the reference tree and the binary that build() leaves under oracle/_ref/"""
    if not (ref_iou3d.reference_present() and ref_iou3d.built()):
        pytest.skip("no reference tree / oracle/_ref binary on this machine")
    for f in G.FAMILIES:
        p = gold[f"{f}/P"]
        got, want = ref_iou3d.boxes_iou_bev(p[:K], p[K:]), gold[f"{f}/iou_ref"]
        assert ((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))).all(), f
    f = G.FAMILIES[2]
    iou, sens, nan = G.reference_and_sensitivity(gold[f"{f}/P"])
    assert np.array_equal(_bits(sens), _bits(gold[f"{f}/sens_full"])) and np.array_equal(nan, gold[f"{f}/nan_full"])
