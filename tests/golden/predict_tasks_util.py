"""Inputs of the six-task predict fixture (tests/golden/make_golden_predict_tasks.py records the reference's outputs for them in
predict_tasks_flip_circle.npz; the tests feed the same seeded maps to this package's CenterHead.predict and to tests/predict_ref.py),
and the seeded map generator the predict tests share."""
import torch

# the six-task nuScenes table and the test_cfg of the circular-NMS configuration (per-task radii), on a NON-SQUARE 40 x 56 map - a
# square one cannot see H and W swapped in a flip - that straddles the centre range in x, y and z
TASKS = [dict(num_class=1, class_names=["car"]), dict(num_class=2, class_names=["truck", "construction_vehicle"]),
         dict(num_class=2, class_names=["bus", "trailer"]), dict(num_class=1, class_names=["barrier"]),
         dict(num_class=2, class_names=["motorcycle", "bicycle"]), dict(num_class=2, class_names=["pedestrian", "traffic_cone"])]
COMMON_HEADS = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}
CFG = dict(post_center_limit_range=[-45.0, -47.0, -2.5, 40.0, 45.0, 2.5], nms=dict(nms_pre_max_size=1000, nms_post_max_size=83, nms_iou_threshold=0.2),
           score_threshold=0.1, pc_range=[-51.2, -51.2], out_size_factor=4, voxel_size=[0.2, 0.2], double_flip=True, circular_nms=True,
           min_radius=[4, 12, 10, 1, 0.85, 0.175])
H, W, SAMPLES, SEED = 40, 56, 2, 4103


def seeded_task_maps(num_cls, seed, h, w, samples, flip, vel=True, peaks=None, peak_logit=(-3.5, 2.0), noise=0.05):
    """Seeded prediction maps [samples (x 4 with flip), C, h, w] of one task, shaped like a trained head's: a heat map far below any
    threshold except at `peaks` cells per sample (default 6 % of the map; one random class each, logit uniform in `peak_logit`), and,
    with flip, four views per sample that agree up to `noise` once mirrored back - view 1 is the scene mirrored along H (reg_y -> 1 - reg_y,
    cos and v_y negated), view 2 along W (reg_x, sin, v_x), view 3 along both."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    hw = h * w
    n = max(1, round(0.06 * hw)) if peaks is None else peaks
    hm = rn(samples, num_cls, hw) * 0.3 - 7.0
    for s in range(samples):
        cells = torch.randperm(hw, generator=g)[:n]
        cls = torch.randint(0, num_cls, (n,), generator=g)
        hm[s, cls, cells] = torch.rand(n, generator=g) * (peak_logit[1] - peak_logit[0]) + peak_logit[0]
    base = dict(reg=torch.rand(samples, 2, h, w, generator=g), height=rn(samples, 1, h, w), dim=rn(samples, 3, h, w) * 0.3 + 0.8,
                rot=rn(samples, 2, h, w), hm=hm.reshape(samples, num_cls, h, w))
    base["vel"] = rn(samples, 2, h, w) * 2   # drawn with or without the branch: the other maps do not depend on `vel`
    if not flip:
        return base if vel else {k: v for k, v in base.items() if k != "vel"}
    out = {}
    for k, v in base.items():
        views = []
        for view in range(4):
            t = v + noise * rn(*v.shape)
            fy, fx = view & 1, view >> 1
            if k == "reg":
                t = torch.stack([1 - t[:, 0] if fx else t[:, 0], 1 - t[:, 1] if fy else t[:, 1]], 1)
            elif k == "rot":   # channel 0 sin, 1 cos
                t = torch.stack([-t[:, 0] if fx else t[:, 0], -t[:, 1] if fy else t[:, 1]], 1)
            elif k == "vel":
                t = torch.stack([-t[:, 0] if fx else t[:, 0], -t[:, 1] if fy else t[:, 1]], 1)
            dims = ([2] if fy else []) + ([3] if fx else [])
            views.append(torch.flip(t, dims) if dims else t)
        out[k] = torch.stack(views, 1).reshape(samples * 4, *v.shape[1:]).contiguous()
    return out if vel else {k: v for k, v in out.items() if k != "vel"}


def predict_tasks_inputs():
    return [seeded_task_maps(t["num_class"], SEED + 100 * i, H, W, SAMPLES, True) for i, t in enumerate(TASKS)]
