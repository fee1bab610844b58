"""Shared by test_eval_ap_cpu.py and test_eval_ap_gpu.py: the fixture tests/golden/eval_ap.npz as annotation lists, random splits whose
decisions are margin-clear, and the overlap-error bound."""
import os

import numpy as np

from sparse2dense_amd import evaluation as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_ap.npz")
CLASSES = ["Car", "Pedestrian", "Cyclist"]
CLASS_INTS = [0, 1, 10]
ZSETS = {1: 1.0, 2: 0.5}
KEYS = ("name", "bbox", "location", "dimensions", "rotation_y", "alpha", "occluded", "truncated")
_cache = {}


def golden():
    if "z" not in _cache:
        _cache["z"] = dict(np.load(GOLDEN))
    return _cache["z"]


def golden_annos():
    """(gt_annos, dt_annos) of the fixture as lists of numpy dictionaries"""
    z = golden()
    out = []
    for prefix, keys in (("gt_", KEYS), ("dt_", KEYS + ("score",))):
        off = z[prefix + "offsets"]
        out.append([{k: z[prefix + k][off[f]:off[f + 1]] for k in keys} for f in range(len(off) - 1)])
    return out


def golden_overlaps(z_axis, metric):
    """the reference's per frame [nd, ng] overlaps"""
    z = golden()
    nd, ng = np.diff(z["dt_offsets"]), np.diff(z["gt_offsets"])
    off = np.concatenate([[0], np.cumsum(nd * ng)])
    flat = z[f"overlaps_z{z_axis}_m{metric}"]
    return [flat[off[f]:off[f + 1]].reshape(nd[f], ng[f]) for f in range(len(nd))]


def to_device(annos, device):
    import torch
    return [{k: (v if k in ("name", "alpha") else torch.from_numpy(np.ascontiguousarray(v)).to(device)) for k, v in a.items()} for a in annos]


def overlap_errors(values, gt_annos, dt_annos, metric, z_axis):
    """(max |values - float64 clip|, max |float64 clip|) over the frames; values: per frame [nd, ng]"""
    err = big = 0.0
    for v, g, d in zip(values, gt_annos, dt_annos):
        exact = E.overlaps64(g, d, metric, z_axis, ZSETS[z_axis])
        err = max(err, np.abs(np.asarray(v, np.float64) - exact).max(initial=0))
        big = max(big, np.abs(exact).max(initial=0))
    return err, big


def assert_overlaps_within_bound(values, gt_annos, dt_annos, metric, z_axis, what):
    """e <= 4 e_reference + 1e-7 max|overlap|, both errors against the float64 clip of the same fp32 rows"""
    e, big = overlap_errors(values, gt_annos, dt_annos, metric, z_axis)
    e_ref, _ = overlap_errors(golden_overlaps(z_axis, metric), gt_annos, dt_annos, metric, z_axis)
    print(f"{what}: metric {metric} z_axis {z_axis}: e = {e:.3e}, e_reference = {e_ref:.3e}, max |overlap| = {big:.3f}")
    assert e <= 4 * e_ref + 1e-7 * big, (what, metric, z_axis, e, e_ref)


def assert_result_equal(got, z, kind):
    assert got["result"] == str(z[kind + "_result"])
    keys = [k for k in z if k.startswith(kind + "_detail/")]
    assert keys and sum(len(v) for v in got["detail"].values()) == len(keys)
    for k in keys:
        _, cls, entry = k.split("/")
        assert np.abs(np.asarray(got["detail"][cls][entry]) - z[k]).max() <= 1e-12, k


# ---- random splits -------------------------------------------------------------------------------------------------------------------
SIZES = {"Car": (4.2, 1.8, 1.6), "Pedestrian": (0.8, 0.7, 1.75), "Cyclist": (1.8, 0.7, 1.7), "Van": (5.0, 2.0, 2.1)}


def random_frame(rng, nd, ng, levels, z_axis=2, cover=False):
    """one frame with exactly nd detections and ng ground truths whose decisions are margin-clear (evaluation.unclear_detections at 1e-3
    for `levels` [K, 3, M]): ground truths on a line, 9 m apart; detections are jittered copies of ground truths (several per ground
    truth when nd > ng, so candidates compete), the unclear ones are replaced by fresh draws.  cover: every ground truth is an easy Car
    and detection i < ng sits close on ground truth i, so the recall reaches 1 and all 41 thresholds are used"""
    names = rng.choice(["Car"] if cover else ["Car", "Car", "Pedestrian", "Cyclist", "Van"], ng)
    gt = dict(name=names.astype("<U16"), bbox=np.zeros((ng, 4)), location=np.zeros((ng, 3)), dimensions=np.zeros((ng, 3)), rotation_y=rng.uniform(-3, 3, ng),
              alpha=np.full(ng, -10.0), occluded=rng.choice(1 if cover else 3, ng), truncated=rng.choice([0.0] if cover else [0.0, 0.2, 0.4], ng))
    for i in range(ng):
        gt["dimensions"][i] = np.array(SIZES[str(names[i])]) * rng.uniform(0.9, 1.1, 3)
        gt["location"][i] = (9.0 * i, rng.uniform(-1, 1), rng.uniform(-0.5, 0.5))
        h = 60.0 if cover else rng.choice([60.0, 33.0, 20.0], p=[0.6, 0.3, 0.1])
        gt["bbox"][i] = (80.0 * i, 100.0, 80.0 * i + 50, 100.0 + h)

    def draw(rows):
        n = len(rows)
        d = dict(name=np.zeros(n, "<U16"), bbox=np.zeros((n, 4)), location=np.zeros((n, 3)), dimensions=np.zeros((n, 3)), rotation_y=np.zeros(n),
                 alpha=np.full(n, -10.0), occluded=np.zeros(n, np.int64), truncated=np.zeros(n), score=np.round(rng.uniform(0.05, 0.99, n), 2))
        for j in range(n):
            close = cover and rows[j] < ng
            if close or (ng and rng.random() < min(0.8, 8.0 * ng / nd)):   # about 8 candidates per ground truth at the most
                i = rows[j] if close else rng.integers(ng)
                shift = 0.03 if close else rng.choice([0.03, 0.08, 0.2, 0.5])
                d["name"][j] = gt["name"][i] if close or rng.random() < 0.85 else "Cyclist"
                d["dimensions"][j] = gt["dimensions"][i] * rng.uniform(0.95, 1.05, 3)
                d["location"][j] = gt["location"][i] + rng.uniform(-shift, shift, 3) * gt["dimensions"][i]
                d["rotation_y"][j] = gt["rotation_y"][i] + rng.uniform(-0.15, 0.15)
                b = gt["bbox"][i]
                du, dv = rng.uniform(-shift, shift, 2) * (b[2] - b[0], b[3] - b[1])
                d["bbox"][j] = (b[0] + du, b[1] + dv, b[2] + du, b[1] + dv + (b[3] - b[1]) * (1.0 if close else rng.choice([1.0, 1.02, 0.5])))
            else:   # a false positive off the line
                d["name"][j] = rng.choice(["Car", "Pedestrian", "Cyclist"])
                d["dimensions"][j] = SIZES[str(d["name"][j])]
                d["location"][j] = (rng.uniform(0, 9.0 * max(ng, 1)), 30.0 + rng.uniform(0, 50), 30.0)
                d["rotation_y"][j] = rng.uniform(-3, 3)
                d["bbox"][j] = (rng.uniform(0, 500), 400.0, 0, 0)
                d["bbox"][j, 2:] = d["bbox"][j, :2] + rng.choice([50.0, 30.0])
        return d
    dt = draw(np.arange(nd))
    for _ in range(20):
        bad = E.unclear_detections(gt, dt, levels, z_axis, ZSETS[z_axis], 1e-3)
        if not bad.any():
            return gt, dt
        fresh = draw(np.nonzero(bad)[0])
        for k in dt:
            dt[k][bad] = fresh[k]
    raise AssertionError("no margin-clear frame found")
