"""Shared by test_gt_sampler_cpu.py and test_gt_sampler_gpu.py: the golden of the reference's GT-database sampler
(tests/golden/gt_sampler.npz, make_golden_gt_sampler.py), its database and stores rebuilt from the arrays, the comparison under the
criteria of frame_prep_util (decisions, names, counts, row order, feature columns and the np.random state exact; coordinates and boxes
within its COORD_ATOL), and seeded random sampler inputs for the comparison of the kernels with the restatement."""
import os

import numpy as np

import frame_prep_util as U

EPS = 2e-3   # collision_clear: no evaluated pair may depend on sizes within 2 mm
GROUPS = [dict(VEHICLE=10), dict(PEDESTRIAN=6), dict(CYCLIST=4)]
PREP_STEPS = [dict(filter_by_min_num_points=dict(VEHICLE=5, PEDESTRIAN=5, CYCLIST=5)), dict(filter_by_difficulty=[-1])]
CASE_TAG = {"1": "n", "2": "s", "3": "n", "4": "n", "5": "n"}


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "gt_sampler.npz")))


def database(g, tag):
    """(db_infos, rows by path, completed clouds by name) of the 9-column ("n") or 7-column ("s") database"""
    names, signs, off, cco = g[f"{tag}_db_names"], g[f"{tag}_db_signs"], g[f"{tag}_db_row_offsets"], g[f"{tag}_db_cc_offsets"]
    db, rows, completed = {}, {}, {}
    for j, (name, sign) in enumerate(zip(names, signs)):
        name, sign = str(name), str(sign)
        info = dict(name=name, path=f"gt_database/{sign}.bin", box3d_lidar=g[f"{tag}_db_boxes"][j].copy(),
                    num_points_in_gt=int(g[f"{tag}_db_num_points"][j]), difficulty=int(g[f"{tag}_db_difficulty"][j]), gt_signs=sign)
        db.setdefault(name, []).append(info)
        rows[info["path"]] = g[f"{tag}_db_rows"][off[j]:off[j + 1]]
        if cco[j + 1] > cco[j]:
            completed[sign] = g[f"{tag}_db_cc"][cco[j]:cco[j + 1]]
    return db, rows, completed


def frame(g, case):
    pre = "c5_frame_" if case == "5" else CASE_TAG[case] + "_frame_"
    f = {k: g[pre + k] for k in ("points", "boxes", "names", "signs")}
    f["objects"] = {}
    if pre + "obj_offsets" in g:
        off = g[pre + "obj_offsets"]
        f["objects"] = {str(s): g[pre + "obj_points"][off[j]:off[j + 1]] for j, s in enumerate(f["signs"]) if off[j + 1] > off[j]}
    return f


def case_cfg(g, case):
    nine = CASE_TAG[case] == "n"
    return dict(mode="train", shuffle_points=True, distillation=nine, global_rot_noise=[-0.78539816, 0.78539816], global_scale_noise=[0.95, 1.05],
                global_translate_std=[0.2, 0.3, 0.1] if nine else 0, class_names=[str(n) for n in g["class_names"]], db_sampler=None,
                no_augmentation=False)


def case_seed(g, case):
    return int(g["seed"]) + {"4": 1, "5": 2}.get(case, 0)


def case_groups(g, case):
    return [dict(VEHICLE=6), dict(PEDESTRIAN=2), dict(CYCLIST=1)] if case == "4" else GROUPS


def build_sampler(g, case, resident=None, convert=lambda a: a):
    """seeds np.random as the generator did and builds the sampler of `case`; returns (sampler, object store over the frame's and the
    database's completed clouds)"""
    from sparse2dense_amd import prep
    db, rows, completed = database(g, CASE_TAG[case])
    f = frame(g, case)
    store = {k: convert(v) for k, v in {**completed, **f["objects"]}.items()}
    np.random.seed(case_seed(g, case))
    sampler = prep.GTSampler(db, case_groups(g, case), rate=1.0, db_prep_steps=PREP_STEPS, points_of=lambda info: rows[info["path"]],
                             global_rot_range=[0, 0])
    if resident is not None:   # (device, with the completed clouds)
        sampler.resident(resident[0], object_store=store.get if resident[1] else None)
    return sampler, store, f


def rng_words():
    state = np.random.get_state()
    return np.concatenate([state[1], [state[2]]]).astype(np.int64)


def kept(f):
    keep = np.array([str(n) not in ("DontCare", "ignore", "UNKNOWN") for n in f["names"]])
    return f["boxes"][keep], f["names"][keep]


def check_sample(got, g, pre):
    """sample_all's dictionary against the recorded one"""
    assert [str(n) for n in got["gt_names"]] == [str(n) for n in g[pre + "gt_names"]]
    assert np.array_equal(got["difficulty"], g[pre + "difficulty"]) and np.array_equal(got["group_ids"], g[pre + "group_ids"])
    assert got["gt_masks"].dtype == np.bool_ and np.array_equal(got["gt_masks"], g[pre + "gt_masks"])
    assert got["gt_boxes"].dtype == np.float32 and np.array_equal(got["gt_boxes"], g[pre + "gt_boxes"])
    U.check_cloud(got["points"], g[pre + "points"], pre + "points")
    U.check_cloud(got["recon_points"], g[pre + "recon_points"], pre + "recon_points")


def check_step(lidar, g, pre, distillation):
    """the outputs of one S2DPreprocess call against one recorded Preprocess call, the np.random state included"""
    assert np.array_equal(rng_words(), g[pre + "rng"]), "np.random state differs from the reference's"
    U.check_cloud(lidar["points"], g[pre + "points"], pre + "points")
    if distillation:
        U.check_cloud(lidar["dense_points"], g[pre + "dense_points"], pre + "dense_points")
        U.check_cloud(lidar["reconstruction_points"], g[pre + "reconstruction_points"], pre + "reconstruction_points")
    anno = lidar["annotations"]
    assert [str(n) for n in anno["gt_names"]] == [str(n) for n in g[pre + "gt_names"]]
    assert np.array_equal(anno["gt_classes"], g[pre + "gt_classes"]) and anno["gt_classes"].dtype == np.int32
    got = U.to_numpy(anno["gt_boxes"])
    assert got.shape == g[pre + "gt_boxes"].shape
    err = np.abs(got.astype(np.float64) - g[pre + "gt_boxes"]).max() if got.size else 0.0
    print(f"{pre}gt_boxes: max error {err:.3e}")
    assert err <= U.COORD_ATOL


def run_case(g, case, convert, resident=None):
    """case 1, 2, 4 or 5 (one frame) or 3 (three frames through one sampler) through S2DPreprocess"""
    from sparse2dense_amd import prep
    sampler, store, f = build_sampler(g, case, resident, convert)
    cfg = case_cfg(g, case)
    step = prep.S2DPreprocess(cfg, object_store=store.get, db_sampler=sampler)
    prefixes = ["c1_full_", "c3_frame2_", "c3_frame3_"] if case == "3" else [f"c{case}_full_"]
    for pre in prefixes:
        res = dict(type="WaymoDataset", lidar=dict(points=convert(f["points"].copy()), annotations=dict(boxes=f["boxes"].copy(), names=f["names"].copy())))
        info = dict(gt_boxes=f["boxes"].copy(), gt_names=f["names"].copy(), gt_signs=[str(s) for s in f["signs"]])
        res, _ = step(res, info)
        check_step(res["lidar"], g, pre, cfg["distillation"])
    return sampler


# ---- seeded random sampler inputs ------------------------------------------------------------------------------------------------
def random_input(seed, m, s, groups, ncols=5, box_dim=7, field=150.0, chain=False, crowd=None, rows=(1, 40)):
    """m frame boxes and s candidates in `groups` groups on a field x field square with boxes of at most 5 m; every candidate has sweep rows
    (0 .. rows[1] - 1 of them when rows[0] == 0), about two thirds a completed cloud with rows outside the box (about one in ten wholly
    outside; rows whose image comes within 5 mm of a face of the box are left out), half are VEHICLEs.  chain: candidate i crosses candidate i + 1 and nothing else (one group).  crowd: "all" packs everything
    into 12 m so that (nearly) everything collides, "none" puts the boxes on a grid with no overlap."""
    rs = np.random.RandomState(seed)
    n = m + s
    boxes = np.zeros((n, box_dim), np.float32)
    boxes[:, :2] = rs.uniform(-field / 2, field / 2, (n, 2))
    boxes[:, 2] = rs.uniform(-1, 2, n)
    boxes[:, 3:6] = rs.uniform(0.5, 5.0, (n, 3))
    if box_dim > 7:
        boxes[:, 6:8] = rs.normal(0, 3, (n, 2))
    boxes[:, -1] = rs.uniform(-4, 4, n)
    if crowd == "all":
        boxes[:, :2] = rs.uniform(-6, 6, (n, 2))
        boxes[:, 3:5] = rs.uniform(3.0, 5.0, (n, 2))
    if crowd == "none":
        side = int(np.ceil(np.sqrt(n)))
        boxes[:, 0], boxes[:, 1] = (np.arange(n) % side) * 8.0 - 4.0 * side, (np.arange(n) // side) * 8.0 - 4.0 * side
    if chain:   # 3.2 x 0.5 m boxes 1.75 m apart along x at y = 200, every second one turned by a right angle: an even box (x +-1.6) pokes 0.1 m
        #           into both odd neighbours (x +-0.25, y +-1.6), even boxes are 0.3 m apart, odd ones 3 m
        boxes[m:, 0], boxes[m:, 1] = np.arange(s) * 1.75 - 0.875 * s, 200.0
        boxes[m:, 3], boxes[m:, 4], boxes[m:, -1] = 3.2, 0.5, np.where(np.arange(s) % 2 == 0, 0.0, np.pi / 2)
    ends = np.sort(rs.choice(np.arange(1, s), groups - 1, replace=False)).tolist() + [s] if groups > 1 else [s]
    kinds = rs.choice([0, 1], s).astype(np.int8)
    src, cc = [], []
    for i in range(s):
        b = boxes[m + i].astype(np.float64)
        k = int(rs.randint(rows[0], rows[1]))
        src.append(np.concatenate([rs.uniform(-1, 1, (k, 3)) * b[3:6] / 2, rs.uniform(0.01, 1, (k, ncols - 3))], 1).astype(np.float32))
        if rs.uniform() < 0.67:
            k = int(rs.randint(1, 60))
            gcl = np.concatenate([rs.uniform(-1, 1, (k, 3)) * b[[4, 3, 5]] / 2 * 0.9, rs.uniform(0.01, 1, (k, ncols - 3))], 1)
            gcl[rs.uniform(0, 1, k) < 0.25, :3] *= 5.0
            gcl[rs.uniform(0, 1, k) < 0.1, 1] = 0.0
            if rs.uniform() < 0.1:
                gcl[:, 2] += 20.0
            cc.append(away_from_faces(gcl.astype(np.float32), boxes[m + i]))
        else:
            cc.append(None)
    return dict(avoid=boxes[:m], cand=boxes[m:], ends=np.asarray(ends, np.int32), kinds=kinds, src=src, cc=cc)


def away_from_faces(g, box):
    """the rows of a completed cloud whose image and mirror image keep 5 mm from every face of the object's box (float64)"""
    from sparse2dense_amd import prep
    a = np.pi / 2 + float(box[-1])
    keep = np.ones(len(g), bool)
    for sgn in (1.0, -1.0):
        x, y = g[:, 0].astype(np.float64), sgn * g[:, 1].astype(np.float64)
        w = np.stack([x * np.cos(a) + y * np.sin(a), -x * np.sin(a) + y * np.cos(a), g[:, 2].astype(np.float64)], 1) + box[:3].astype(np.float64)
        keep &= np.abs(prep.face_distance(w, box[None])[:, 0]) >= 5e-3
    return g[keep] if keep.any() else None


def sampler_of(inp):
    """a GTSampler whose next draw is exactly the candidates of `inp`, in order: one class per group, as many entries as the group draws + 1
    (so that no draw wraps), max_num = the group's size (the frame's names are to name none of the classes G0, G1, ...)"""
    from sparse2dense_amd import prep
    db, groups, start = {}, [], 0
    for gi, end in enumerate(inp["ends"]):
        infos = [dict(name="VEHICLE" if inp["kinds"][i] == 1 else "PEDESTRIAN", path=str(i), box3d_lidar=inp["cand"][i].copy(),
                      num_points_in_gt=len(inp["src"][i]), difficulty=0, gt_signs=f"cand_{i}") for i in range(start, end)]
        infos.append(dict(infos[-1], path="spare", gt_signs="spare"))
        db[f"G{gi}"] = infos
        groups.append({f"G{gi}": int(end - start)})
        start = end
    rows = {str(i): r for i, r in enumerate(inp["src"])}
    rows["spare"] = inp["src"][0]
    sampler = prep.GTSampler(db, groups, points_of=lambda info: rows[info["path"]])
    for smp in sampler._samplers.values():   # the identity order: the next draw of every class is its first entries
        smp.indices = np.arange(smp.n)
    store = {f"cand_{i}": g for i, g in enumerate(inp["cc"]) if g is not None}
    return sampler, store


def unclear_pairs(inp):
    """pairs the selection can evaluate (candidate rows against every box) that are not collision_clear at EPS"""
    from sparse2dense_amd import prep
    total = np.concatenate([inp["avoid"], inp["cand"]], 0)
    clear = prep.collision_clear(inp["cand"], total, EPS)
    m = len(inp["avoid"])
    clear[np.arange(len(inp["cand"])), m + np.arange(len(inp["cand"]))] = True
    return int((~clear).sum())
