"""Shared by test_frame_prep_cpu.py and test_frame_prep_gpu.py: the golden of the reference's frame preparation
(tests/golden/frame_prep.npz, make_golden_frame_prep.py), the comparison criteria, and seeded random frames.

Criteria (the same on both paths): masks, counts, row counts, row order and the intensity / elongation columns equal; coordinates and
box columns within COORD_ATOL = 1e-4 m absolute.  Why 1e-4: each coordinate is a three-term fp32 product sum of values up to 128 (one
fp32 ulp there is 1.5e-5) plus a scale and a translate; each of the two fp32 evaluations can be off by a few half-ulps, and six half-ulps
each give about 9e-5 between them.  Row order is compared through the feature columns, which are continuous random values (distinct).
"""
import os

import numpy as np

COORD_ATOL = 1e-4
NEAR_FACE = 1e-3
CASES = ("a", "b", "c")


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "frame_prep.npz")))


def to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def check_cloud(got, want, what):
    got, want = to_numpy(got), np.asarray(want)
    assert got.dtype == np.float32, (what, got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:, 3:], want[:, 3:]), f"{what}: rows or row order differ"
    err = np.abs(got[:, :3].astype(np.float64) - want[:, :3]).max() if len(want) else 0.0
    print(f"{what}: {got.shape[0]} rows, max coordinate error {err:.3e}")
    assert err <= COORD_ATOL, (what, err)


def case_cfg(g, tag, **over):
    rot, std = g[f"{tag}_rot"], g[f"{tag}_std"]
    cfg = dict(mode="train", shuffle_points=bool(g[f"{tag}_shuffle"]), distillation=True, global_rot_noise=rot.tolist() if rot.ndim else float(rot),
               global_scale_noise=[0.95, 1.05], global_translate_std=std.tolist() if std.ndim else float(std),
               class_names=[str(n) for n in g["class_names"]], db_sampler=None, no_augmentation=False)
    cfg.update(over)
    return cfg


KINDS = {"full": {}, "comp": dict(no_augmentation=True, shuffle_points=False), "plain": dict(distillation=False)}


def case_store(g, tag, convert):
    off = g[f"{tag}_obj_offsets"]
    return {str(s): convert(g[f"{tag}_obj_points"][off[j]:off[j + 1]]) for j, s in enumerate(g[f"{tag}_signs"]) if off[j + 1] > off[j]}


def run_case(g, tag, kind, convert):
    """the reference's run `kind` of case `tag` through S2DPreprocess; `convert` places the sweep and the stored clouds (numpy -> numpy for
    the restatement, numpy -> CUDA tensor for the kernels).  Compares everything the golden holds, the MT19937 state included."""
    from sparse2dense_amd import prep
    cfg = case_cfg(g, tag, **KINDS[kind])
    boxes, names = g[f"{tag}_boxes"], g[f"{tag}_names"]
    step = prep.S2DPreprocess(cfg, object_store=case_store(g, tag, convert).get)
    res = dict(type="WaymoDataset", lidar=dict(points=convert(g[f"{tag}_points"].copy()), annotations=dict(boxes=boxes.copy(), names=names.copy())))
    info = dict(gt_boxes=boxes.copy(), gt_names=names.copy(), gt_signs=[str(s) for s in g[f"{tag}_signs"]])
    np.random.seed(int(g[f"{tag}_seed"]))
    res, _ = step(res, info)
    state = np.random.get_state()
    lidar, pre = res["lidar"], f"{tag}_{kind}_"
    assert np.array_equal(np.concatenate([state[1], [state[2]]]).astype(np.int64), g[pre + "rng"]), "np.random state differs from the reference's"
    check_cloud(lidar["points"], g[pre + "points"], pre + "points")
    if cfg["distillation"]:
        check_cloud(lidar["dense_points"], g[pre + "dense_points"], pre + "dense_points")
        check_cloud(lidar["reconstruction_points"], g[pre + "reconstruction_points"], pre + "reconstruction_points")
    else:
        assert "dense_points" not in lidar
    anno = lidar["annotations"]
    assert [str(n) for n in anno["gt_names"]] == [str(n) for n in g[pre + "gt_names"]]
    assert np.array_equal(anno["gt_classes"], g[pre + "gt_classes"]) and anno["gt_classes"].dtype == np.int32
    got = to_numpy(anno["gt_boxes"])
    assert got.shape == g[pre + "gt_boxes"].shape
    err = np.abs(got.astype(np.float64) - g[pre + "gt_boxes"]).max() if got.size else 0.0
    print(f"{pre}gt_boxes: max error {err:.3e}")
    assert err <= COORD_ATOL


def random_frame(seed, n, m, stored="some", inside="mix", long_object=False, box_dim=7):
    """a seeded frame at the given sizes: boxes spread over +-70 m, the sweep a mix of background and points in and around the boxes
    (`inside` "all": every point inside a box, "none": no point inside any), stored clouds for "some" / "all" / "none" of the boxes that are
    no SIGN - some rows far outside their box, VEHICLEs with unequal sides and y == 0 rows - and with long_object one VEHICLE of 700 rows
    and one other object of 300 (more than a 256-row tile).  Sweep points closer than 5 mm to a box surface are drawn again."""
    from sparse2dense_amd import prep
    rs = np.random.RandomState(seed)
    boxes = np.zeros((m, box_dim), np.float32)
    boxes[:, :2] = rs.uniform(-70, 70, (m, 2))
    boxes[:, 2] = rs.uniform(-1, 2, m)
    boxes[:, 3:6] = rs.uniform(0.5, 5.0, (m, 3))
    if box_dim > 7:
        boxes[:, 6:8] = rs.normal(0, 3, (m, 2))
    boxes[:, -1] = rs.uniform(-4, 4, m)
    kinds = rs.choice([0, 1, 1, 2], m).astype(np.int8)
    if long_object:
        kinds[0], kinds[1] = 1, 0

    def draw(k):
        if m == 0 or inside == "none":
            p = np.concatenate([rs.uniform(-75, 75, (k, 2)), rs.uniform(-2, 4, (k, 1))], 1)
        else:
            j = rs.randint(0, m, k)
            b = boxes[j].astype(np.float64)
            loc = rs.uniform(-1, 1, (k, 3)) * b[:, 3:6] / 2 * (0.95 if inside == "all" else 1.3)
            c, s = np.cos(b[:, -1]), np.sin(b[:, -1])
            p = np.stack([loc[:, 0] * c + loc[:, 1] * s, -loc[:, 0] * s + loc[:, 1] * c, loc[:, 2]], 1) + b[:, :3]
            if inside == "mix":
                bg = rs.uniform(0, 1, k) < 0.5
                p[bg] = np.concatenate([rs.uniform(-75, 75, (k, 2)), rs.uniform(-2, 4, (k, 1))], 1)[bg]
        return np.concatenate([p, rs.uniform(0, 1, (k, 2))], 1).astype(np.float32)
    points = draw(n)
    for _ in range(20):
        if n == 0 or m == 0:
            break
        d = prep.face_distance(points, boxes)
        bad = (np.abs(d) < 5e-3).any(1)
        if inside == "none":
            bad |= (d < 0).any(1)
        if not bad.any():
            break
        points[bad] = draw(int(bad.sum()))
    objects = []
    for j in range(m):
        has = kinds[j] != 2 and (stored == "all" or (stored == "some" and rs.uniform() < 0.6))
        if not has:
            objects.append(np.zeros((0, 5), np.float32))
            continue
        k = int(rs.randint(1, 40))
        if long_object and j < 2:
            k = (700, 300)[j]
        half = boxes[j, [4, 3, 5]].astype(np.float64) / 2
        g = np.concatenate([rs.uniform(-1, 1, (k, 3)) * half * 0.9, rs.uniform(0, 1, (k, 2))], 1)
        far = rs.uniform(0, 1, k) < 0.2
        g[far, :3] *= 6.0
        g[rs.uniform(0, 1, k) < 0.1, 1] = 0.0
        objects.append(g.astype(np.float32))
    obj_points = np.concatenate(objects, 0) if objects else np.zeros((0, 5), np.float32)
    obj_offsets = np.cumsum([0] + [len(g) for g in objects]).astype(np.int32)
    return dict(points=points, boxes=boxes, kinds=kinds, obj_points=obj_points.astype(np.float32), obj_offsets=obj_offsets)
