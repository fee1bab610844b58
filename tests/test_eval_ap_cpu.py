"""Detection AP evaluation, host side: `sparse2dense_amd.evaluation` (the float64 definition and the route of CPU inputs) against
tests/golden/eval_ap.npz, which holds what the reference's own evaluator returns for the same annotations
(tests/golden/make_golden_eval_ap.py).  The scenes' decisions are margin-clear, so precisions, thresholds and mAP are compared to 1e-12
and the result strings exactly; the overlaps are compared within the bound of eval_ap_util.assert_overlaps_within_bound."""
import numpy as np
import pytest

import eval_ap_util as U
from sparse2dense_amd import evaluation as E


@pytest.fixture(scope="module")
def annos():
    return U.golden_annos()


def test_fixture_is_margin_clear(annos):
    gt, dt = annos
    levels = np.concatenate([E.official_min_overlaps(U.CLASSES), E.coco_min_overlaps(U.CLASSES)], 0)
    for z_axis, z_center in U.ZSETS.items():
        assert E.decisions_clear(gt, dt, levels, z_axis, z_center, 1e-3)
    counts = [(len(g["name"]), len(d["name"])) for g, d in zip(gt, dt)]
    assert any(g and not d for g, d in counts) and any(d and not g for g, d in counts) and (0, 0) in counts
    names = set(np.concatenate([g["name"] for g in gt]))
    assert {"Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare"} <= names


@pytest.mark.parametrize("z_axis", [1, 2])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_overlaps(annos, metric, z_axis):
    gt, dt = annos
    mine, _, total_dt, total_gt = E.calculate_iou_partly(dt, gt, metric, z_axis=z_axis, z_center=U.ZSETS[z_axis])
    assert [m.shape for m in mine] == [o.shape for o in U.golden_overlaps(z_axis, metric)]
    assert total_dt.tolist() == [len(d["name"]) for d in dt] and total_gt.tolist() == [len(g["name"]) for g in gt]
    U.assert_overlaps_within_bound(mine, gt, dt, metric, z_axis, "host definition")


@pytest.mark.parametrize("z_axis", [1, 2])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_eval_class(annos, metric, z_axis):
    gt, dt = annos
    z = U.golden()
    before = dict(E.eval_paths)
    ret = E.eval_class_v3(gt, dt, U.CLASS_INTS, (0, 1, 2), metric, E.official_min_overlaps(U.CLASSES), False, z_axis=z_axis,
                          z_center=U.ZSETS[z_axis])
    assert E.eval_paths["host"] == before["host"] + 1 and E.eval_paths["device"] == before["device"]
    for k in ("precision", "thresholds"):
        assert ret[k].shape == (3, 3, 2, 41)
        assert np.abs(ret[k] - z[f"{k}_z{z_axis}_m{metric}"]).max() <= 1e-12
    assert not ret["recall"].any() and not ret["orientation"].any()
    assert np.abs(E.get_mAP(ret["precision"]) - E.get_mAP(z[f"precision_z{z_axis}_m{metric}"])).max() <= 1e-12


def test_thresholds_skip_entries_and_a_class_without_true_positive(annos):
    gt, dt = annos
    ret = E.eval_class_v3(gt, dt, U.CLASS_INTS, (0, 1, 2), 2, E.official_min_overlaps(U.CLASSES), False, z_axis=2, z_center=0.5)
    assert ret["counts"][0, 2, 1, :, 0].max() > 40 > (ret["thresholds"][0, 2, 1] > 0).sum()
    assert ret["counts"][2, :, :, :, 0].max() == 0 and not ret["precision"][2].any()


def test_orientation(annos):
    gt, dt = annos
    z = U.golden()
    d_off, g_off = z["dt_offsets"], z["gt_offsets"]
    dt = [dict(d, alpha=z["aos_dt_alpha"][d_off[f]:d_off[f + 1]]) for f, d in enumerate(dt)]
    gt = [dict(g, alpha=z["aos_gt_alpha"][g_off[f]:g_off[f + 1]]) for f, g in enumerate(gt)]
    assert E.compute_aos_of(dt)
    ret = E.eval_class_v3(gt, dt, U.CLASS_INTS, (0, 1, 2), 0, E.official_min_overlaps(U.CLASSES), True, z_axis=2, z_center=0.5)
    assert z["aos_orientation"].max() > 0
    assert np.abs(ret["orientation"] - z["aos_orientation"]).max() <= 1e-12
    assert np.abs(ret["precision"] - z["aos_precision"]).max() <= 1e-12


def test_official_and_coco_results(annos):
    gt, dt = annos
    z = U.golden()
    U.assert_result_equal(E.get_official_eval_result(gt, dt, U.CLASSES, z_axis=2, z_center=0.5), z, "official")
    U.assert_result_equal(E.get_coco_eval_result(gt, dt, U.CLASSES, z_axis=2, z_center=0.5), z, "coco")


def test_statistics_scan_matches_the_literal_loop(annos):
    """the reduction of compute_statistics_jit against the reference's detection loop written out, on the fixture's frames"""
    gt, dt = annos

    def literal(overlaps, dt_scores, ignored_gt, ignored_det, min_overlap, thresh, compute_fp):
        no, assigned, tp, fn, picked = -10000000, [False] * len(dt_scores), 0, 0, []
        below = [compute_fp and s < thresh for s in dt_scores]
        for i in range(len(ignored_gt)):
            if ignored_gt[i] == -1:
                continue
            det_idx, valid, max_overlap, assigned_ignored = -1, no, 0, False
            for j in range(len(dt_scores)):
                if ignored_det[j] == -1 or assigned[j] or below[j]:
                    continue
                overlap = overlaps[j, i]
                if not compute_fp and overlap > min_overlap and dt_scores[j] > valid:
                    det_idx, valid = j, dt_scores[j]
                elif compute_fp and overlap > min_overlap and (overlap > max_overlap or assigned_ignored) and ignored_det[j] == 0:
                    max_overlap, det_idx, valid, assigned_ignored = overlap, j, 1, False
                elif compute_fp and overlap > min_overlap and valid == no and ignored_det[j] == 1:
                    det_idx, valid, assigned_ignored = j, 1, True
            if valid == no and ignored_gt[i] == 0:
                fn += 1
            elif valid != no and (ignored_gt[i] == 1 or ignored_det[det_idx] == 1):
                assigned[det_idx] = True
            elif valid != no:
                tp += 1
                picked.append(dt_scores[det_idx])
                assigned[det_idx] = True
        return tp, fn, picked

    overlaps = E.calculate_iou_partly(dt, gt, 2, z_axis=2, z_center=0.5)[0]
    checked = 0
    for cls in U.CLASS_INTS:
        for diff in (0, 2):
            rets = E.prepare_data(gt, dt, cls, diff)
            for f in range(len(gt)):
                for min_overlap in (0.25, 0.7):
                    for compute_fp, thresh in ((False, 0.0), (True, 0.3)):
                        tp, fp, fn, _, picked = E.compute_statistics_jit(overlaps[f], rets[0][f], rets[1][f], rets[2][f], rets[3][f], rets[4][f], 2,
                                                                         min_overlap, thresh, compute_fp)
                        want = literal(overlaps[f], rets[1][f][:, -1], rets[2][f], rets[3][f], min_overlap, thresh, compute_fp)
                        assert (tp, fn, picked.tolist()) == want
                        checked += tp
    assert checked > 100


def test_routing_reasons_and_counters(annos, monkeypatch):
    gt, dt = annos
    assert E.device_reason(gt, dt) == "annotations on the host"
    assert E.device_reason([], []) == "annotations on the host"
    monkeypatch.setenv("S2D_EVAL_DEVICE", "0")
    assert E.device_reason(gt, dt) == "S2D_EVAL_DEVICE=0"
    monkeypatch.delenv("S2D_EVAL_DEVICE")
    before = dict(E.eval_paths)
    E.get_official_eval_result(gt[:2], dt[:2], ["Car"], z_axis=2, z_center=0.5)
    assert E.eval_paths == {"host": before["host"] + 3, "device": before["device"]}
    assert set(E.eval_paths) == {"device", "host"}


def test_name_codes_round_trip():
    names = ["Car", "car", "Van", "Person_sitting", "DontCare", "ignore", "Tram", "traffic_cone", "Cyclist"]
    codes = E.name_codes(names)
    assert codes.tolist() == [0, 0, 11, 12, 15 | 256, 15 | 256, 15, 9, 10]
    back = E.names_of_codes(codes)
    assert E.name_codes(back).tolist() == codes.tolist()


def test_shim_names_resolve():
    from sparse2dense_amd import det3d_shim
    det3d_shim.install()
    import importlib
    kitti = importlib.import_module("det3d.datasets.kitti.eval")
    for name in ("get_thresholds", "clean_data", "eval_class_v3", "get_mAP", "do_eval_v3", "do_coco_style_eval", "get_official_eval_result",
                 "get_coco_eval_result"):
        assert getattr(kitti, name) is getattr(E, name)
    utils = importlib.import_module("det3d.datasets.utils.eval")
    for name in ("calculate_iou_partly", "compute_statistics_jit", "prepare_data", "bev_box_overlap", "box3d_overlap", "image_box_overlap"):
        assert getattr(utils, name) is getattr(E, name)
    from det3d.ops.nms.nms_gpu import rotate_iou_gpu_eval
    assert rotate_iou_gpu_eval is E.rotate_iou_gpu_eval


def test_entries_are_declared_and_bound():
    """the three entries are in include/s2d.h and _lib.SIGNATURES (test_cabi.test_header_symbols_all_exported compares the two sets), and
    none is a workspace query (test_ws_guard_cpu pins that set of names)"""
    import test_cabi
    from sparse2dense_amd import _lib
    new = {"s2d_eval_overlaps", "s2d_eval_match", "s2d_eval_pr"}
    assert new <= set(test_cabi.declared_symbols(("s2d.h",))) and new <= set(_lib.SIGNATURES)
    assert {n for n in _lib.SIGNATURES if "eval" in n} == new
    assert not [n for n in new if n.endswith(("_workspace_bytes", "_workspace_floats"))]
