"""Detection AP evaluation on the device (csrc/eval_ap.hip through sparse2dense_amd.evaluation): the fixture of the reference's evaluator
and random margin-clear splits against the host definition.  Decisions are margin-clear (evaluation.unclear_detections at 1e-3), so
thresholds and precisions are compared to 1e-12 and the tp / fp / fn counts as integers; the overlaps within
eval_ap_util.assert_overlaps_within_bound."""
import numpy as np
import pytest
import torch

import eval_ap_util as U
from sparse2dense_amd import evaluation as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def annos():
    gt, dt = U.golden_annos()
    return gt, dt, U.to_device(gt, DEV), U.to_device(dt, DEV)


def assert_same_eval(got, want):
    assert np.array_equal(got["counts"], want["counts"]) and got["counts"].dtype == np.int64
    for k in ("precision", "thresholds"):
        assert np.abs(got[k] - want[k]).max() <= 1e-12, k
    assert not got["recall"].any() and not got["orientation"].any()


def both_routes(gt, dt, classes, difficultys, metric, levels, z_axis=2):
    """(device result, host result) of eval_class_v3, with the routes checked by the counters"""
    before = dict(E.eval_paths)
    dev = E.eval_class_v3(U.to_device(gt, DEV), U.to_device(dt, DEV), classes, difficultys, metric, levels, False, z_axis=z_axis,
                          z_center=U.ZSETS[z_axis])
    assert E.eval_paths == {"device": before["device"] + 1, "host": before["host"]}
    host = E.eval_class_v3(gt, dt, classes, difficultys, metric, levels, False, z_axis=z_axis, z_center=U.ZSETS[z_axis])
    assert E.eval_paths == {"device": before["device"] + 1, "host": before["host"] + 1}
    return dev, host


@pytest.mark.parametrize("z_axis", [1, 2])
def test_fixture_overlaps(annos, z_axis):
    gt, dt, gt_d, dt_d = annos
    assert E.device_reason(gt_d, dt_d) is None
    packed = E._Packed(gt_d, dt_d)
    for metric in range(3):
        mine = E.frame_overlaps(packed, E.device_overlaps(packed, metric, z_axis, U.ZSETS[z_axis]))
        assert [m.shape for m in mine] == [o.shape for o in U.golden_overlaps(z_axis, metric)]
        U.assert_overlaps_within_bound(mine, gt, dt, metric, z_axis, "device")
    assert packed.launches == 3 and packed.host_reads == 0


@pytest.mark.parametrize("z_axis", [1, 2])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_fixture_eval_class(annos, metric, z_axis):
    gt, dt, gt_d, dt_d = annos
    z = U.golden()
    levels = E.official_min_overlaps(U.CLASSES)
    packed = E._Packed(gt_d, dt_d)
    ret = E.eval_class_v3(gt_d, dt_d, U.CLASS_INTS, (0, 1, 2), metric, levels, False, z_axis=z_axis, z_center=U.ZSETS[z_axis], _packed=packed)
    assert (packed.launches, packed.host_reads) == (E.EVAL_CLASS_LAUNCHES, E.EVAL_CLASS_HOST_READS) == (3, 2)
    for k in ("precision", "thresholds"):
        assert np.abs(ret[k] - z[f"{k}_z{z_axis}_m{metric}"]).max() <= 1e-12
    host = E.eval_class_v3(gt, dt, U.CLASS_INTS, (0, 1, 2), metric, levels, False, z_axis=z_axis, z_center=U.ZSETS[z_axis])
    assert_same_eval(ret, host)
    assert host["counts"][..., 0].max() > 0 and (metric != 0 or host["counts"][..., 1].max() > 0)


def test_fixture_results(annos):
    _, _, gt_d, dt_d = annos
    z = U.golden()
    before = dict(E.eval_paths)
    U.assert_result_equal(E.get_official_eval_result(gt_d, dt_d, U.CLASSES, z_axis=2, z_center=0.5), z, "official")
    U.assert_result_equal(E.get_coco_eval_result(gt_d, dt_d, U.CLASSES, z_axis=2, z_center=0.5), z, "coco")
    assert E.eval_paths == {"device": before["device"] + 6, "host": before["host"]}


def test_switch_and_orientation_take_the_host(annos, monkeypatch):
    _, _, gt_d, dt_d = annos
    assert "compute_aos" in E.device_reason(gt_d, dt_d, compute_aos=True)
    assert "negative" in E.device_reason(gt_d, dt_d, min_overlaps=np.array([[[-0.1]]]))
    monkeypatch.setenv("S2D_EVAL_DEVICE", "0")
    assert E.device_reason(gt_d, dt_d) == "S2D_EVAL_DEVICE=0"
    before = dict(E.eval_paths)
    ret = E.eval_class_v3(gt_d, dt_d, U.CLASS_INTS, (0, 1, 2), 1, E.official_min_overlaps(U.CLASSES), False, z_axis=2, z_center=0.5)
    assert E.eval_paths == {"device": before["device"], "host": before["host"] + 1}
    assert np.abs(ret["precision"] - U.golden()["precision_z2_m1"]).max() <= 1e-12


def split(rng, nds, ngs, levels, cover=False):
    frames = [U.random_frame(rng, nd, ng, levels, cover=cover) for nd, ng in zip(nds, ngs)]
    return [f[0] for f in frames], [f[1] for f in frames]


def test_one_frame_at_the_limit_one_overlap_value():
    levels = E.official_min_overlaps(U.CLASSES)[:1]
    gt, dt = split(np.random.default_rng(1), [1024], [65], levels)
    for metric in (0, 2):
        dev, host = both_routes(gt, dt, U.CLASS_INTS, (2,), metric, levels)
        assert_same_eval(dev, host)
        assert host["counts"][..., 0].max() > 3 and host["counts"][..., 1].max() > 3


def test_seventy_frames_every_row_count():
    levels = E.official_min_overlaps(U.CLASSES)
    nds, ngs = [[0, 1, 63, 64, 65, 129][f % 6] for f in range(70)], [[0, 1, 33, 65][f % 4] for f in range(70)]
    gt, dt = split(np.random.default_rng(2), nds, ngs, levels)
    dev, host = both_routes(gt, dt, U.CLASS_INTS, (0, 2), 2, levels)
    assert_same_eval(dev, host)
    assert host["counts"][..., 0].max() > 40 and host["counts"][..., 2].max() > 0


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_ten_overlap_values_and_41_thresholds(metric):
    levels = E.coco_min_overlaps(U.CLASSES)
    gt, dt = split(np.random.default_rng(3), [12, 14, 10, 13, 30], [10, 12, 10, 9, 11], levels, cover=True)
    dev, host = both_routes(gt, dt, U.CLASS_INTS, (0, 1, 2), metric, levels)
    assert_same_eval(dev, host)
    used = (host["thresholds"] > 0).sum(-1)
    assert used.max() == 41 and used[0, 0].min() < 41   # every sample point at the low overlaps, fewer at 0.95


def test_a_frame_above_the_limit_takes_the_host():
    levels = E.official_min_overlaps(U.CLASSES)[:1]
    rng = np.random.default_rng(4)
    gt, dt = split(rng, [1025, 3], [65, 4], levels)
    gt_d, dt_d = U.to_device(gt, DEV), U.to_device(dt, DEV)
    assert "1025 detections" in E.device_reason(gt_d, dt_d)
    before = dict(E.eval_paths)
    ret = E.eval_class_v3(gt_d, dt_d, U.CLASS_INTS, (2,), 2, levels, False, z_axis=2, z_center=0.5)
    assert E.eval_paths == {"device": before["device"], "host": before["host"] + 1}
    assert_same_eval(ret, E.eval_class_v3(gt, dt, U.CLASS_INTS, (2,), 2, levels, False, z_axis=2, z_center=0.5))
    many_gt = [dict(gt[1], **{k: np.concatenate([gt[1][k]] * 300) for k in gt[1]})]
    assert len(many_gt[0]["name"]) == 1200 and "1200 ground-truth rows" in E.device_reason(U.to_device(many_gt, DEV), dt_d[1:])
    assert E.device_reason(gt_d[1:], dt_d[1:]) is None


def test_two_calls_give_the_same_bits(annos):
    _, _, gt_d, dt_d = annos
    levels = E.coco_min_overlaps(U.CLASSES)
    runs = []
    for _ in range(2):
        packed = E._Packed(gt_d, dt_d)
        ov = E.device_overlaps(packed, 2, 2, 0.5)
        thresholds, used, pr = E.device_counts(packed, ov, U.CLASS_INTS, (0, 1, 2), 2, levels)
        runs.append((ov.cpu().numpy().tobytes(), thresholds.tobytes(), used.tobytes(), pr.tobytes()))
    assert runs[0] == runs[1]


def test_evaluator_from_tensors_equals_the_dictionaries():
    levels = E.official_min_overlaps(U.CLASSES)
    gt, dt = split(np.random.default_rng(5), [40, 0, 25], [20, 6, 0], levels)
    names = ["Car", "Pedestrian", "Cyclist", "Van"]   # the detector's label order; Van is scored as no class
    ev = E.Evaluator(names, z_axis=2, z_center=0.5)
    dict_gt, dict_dt = [], []
    for g, d in zip(gt, dt):
        box = lambda a: torch.from_numpy(np.concatenate([a["location"], a["dimensions"], a["rotation_y"][:, None]], 1).astype(np.float32)).to(DEV)
        labels = torch.tensor([names.index(n) for n in d["name"]], dtype=torch.int64, device=DEV)
        pred = dict(box3d_lidar=box(d), scores=torch.from_numpy(d["score"].astype(np.float32)).to(DEV), label_preds=labels)
        ev.add([pred], [box(g)], [list(g["name"])])
        fill = lambda a, n: dict(a, bbox=np.tile([0.0, 0.0, 50.0, 50.0], (n, 1)), occluded=np.zeros(n), truncated=np.zeros(n),
                                 location=a["location"].astype(np.float32), dimensions=a["dimensions"].astype(np.float32),
                                 rotation_y=a["rotation_y"].astype(np.float32))
        dict_gt.append(fill(g, len(g["name"])))
        dict_dt.append(dict(fill(d, len(d["name"])), score=d["score"].astype(np.float32)))
    before = dict(E.eval_paths)
    got, coco = ev.official(), ev.coco()
    assert E.eval_paths == {"device": before["device"] + 6, "host": before["host"]}
    want = E.get_official_eval_result(dict_gt, dict_dt, U.CLASSES, [0], z_axis=2, z_center=0.5)
    assert got["result"] == want["result"] and got["detail"] == want["detail"]
    want = E.get_coco_eval_result(dict_gt, dict_dt, U.CLASSES, z_axis=2, z_center=0.5)
    assert coco["result"] == want["result"] and coco["detail"] == want["detail"]
    assert any(v[0] > 0 for v in got["detail"]["car"].values())
