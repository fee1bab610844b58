"""The GT-database sampler without a GPU: the numpy restatement of sparse2dense_amd/prep.py against the golden of the reference's own
`DataBaseSamplerV2` and `Preprocess.__call__` (tests/golden/gt_sampler.npz; criteria: tests/frame_prep_util.py), containment against a
float64 restatement written here (separating axes - the golden holds no containment pair, so that parity is unpinned), the BatchSampler
edges, the argument checks, and the validation of the new C entries (which return before any HIP call)."""
import ctypes

import numpy as np
import pytest
import torch

import gt_sampler_util as G
from sparse2dense_amd import _lib, build, prep


@pytest.fixture(scope="module")
def golden(golden_dir):
    return G.load_golden(golden_dir)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("case", ["1", "2"])
def test_sample_all_restatement_equals_the_reference(golden, case):
    sampler, store, f = G.build_sampler(golden, case)
    boxes, names = G.kept(f)
    got = sampler.sample_all(boxes, names, store.get)
    assert np.array_equal(G.rng_words(), golden[f"c{case}_sample_rng"])
    G.check_sample(got, golden, f"c{case}_sample_")
    assert set(got) == {"gt_names", "difficulty", "gt_boxes", "points", "gt_masks", "recon_points", "group_ids"}


@pytest.mark.parametrize("case", ["1", "2", "3", "4", "5"])
def test_preprocess_restatement_equals_the_reference(golden, case):
    """every cloud, boxes, names, classes and the np.random state after every call; case 3 is three frames through one sampler"""
    sampler = G.run_case(golden, case, lambda a: a)
    if case == "3":   # PEDESTRIAN: 4, exact fit (reset), 4; CYCLIST: 3, 3, a short draw (reset)
        assert sampler._samplers["PEDESTRIAN"].idx == 4 and sampler._samplers["CYCLIST"].idx == 0


def test_the_golden_holds_what_it_must(golden):
    g = golden
    sampler, store, f = G.build_sampler(g, "1")
    boxes, names = G.kept(f)
    drawn = sampler._draw(names)
    assert [(n, len(i)) for n, i in drawn] == [("VEHICLE", 4), ("PEDESTRIAN", 4), ("CYCLIST", 3)]
    cand = np.stack([sampler.db_infos[n][k]["box3d_lidar"] for n, idx in drawn for k in idx])
    accept = prep.GTSampler.select_np(boxes, cand, np.array([4, 8, 11]))
    assert accept.tolist() == [False, False, True, True, True, False, True, True, True, True, True]
    total = np.concatenate([boxes, cand], 0)
    coll = prep.box_collision_test(prep.bev_corners(total), prep.bev_corners(total))
    m = len(boxes)
    assert coll[m + 0, :m].any()                                                    # V0 against a frame box
    assert coll[m + 1, m + 2] and coll[m + 1].sum() == 1 and coll[m + 2].sum() == 1   # V1 rejected because of the later V2 only
    assert coll[m + 4, m + 0] and coll[m + 4].sum() == 1                              # P0 only against the rejected V0
    assert coll[m + 5, m + 3] and coll[m + 5].sum() == 1                              # P1 against the accepted V3
    off = ~np.eye(len(total), dtype=bool)
    assert prep.collision_clear(total, total, G.EPS)[off].all()
    corners = prep._bev_corners_np(total, np.float64)
    assert not (prep._holds_np(corners, corners) & off).any(), "the golden holds no containment pair"
    v3, p2, c2 = sampler.db_infos["VEHICLE"][drawn[0][1][3]], sampler.db_infos["PEDESTRIAN"][drawn[1][1][2]], sampler.db_infos["CYCLIST"][drawn[2][1][2]]
    block = prep._object_block_np(store[v3["gt_signs"]], prep.KIND_VEHICLE, v3["box3d_lidar"])
    inside = prep._inside_np(block, v3["box3d_lidar"][None]).any(1)
    assert 0 < inside.sum() < len(inside) and p2["gt_signs"] not in store
    block = prep._object_block_np(store[c2["gt_signs"]], prep.KIND_OTHER, c2["box3d_lidar"])
    assert len(block) and not prep._inside_np(block, c2["box3d_lidar"][None]).any()
    assert g["c1_full_gt_boxes"].shape[1] == 9 and g["c2_full_gt_boxes"].shape[1] == 7
    assert len(g["c4_full_points"]) == len(g["n_frame_points"]) and not g["c5_full_reconstruction_points"][-1, 3:].any()
    assert len(sampler.db_infos["VEHICLE"]) == 40 and len(sampler.db_infos["PEDESTRIAN"]) == 8 and len(sampler.db_infos["CYCLIST"]) == 7


# ---- containment: a float64 restatement by separating axes, written independently of prep.py ------------------------------------------
def overlap_f64(a, b):
    """open rectangles a and b ([x, y, dx, dy, yaw], the reference's corner convention) intersect: no axis of either separates them"""
    def corners(r):
        x, y, dx, dy, yaw = r
        c, s = np.cos(yaw), np.sin(yaw)
        loc = np.array([[-dx, -dy], [-dx, dy], [dx, dy], [dx, -dy]]) / 2
        return np.stack([loc[:, 0] * c + loc[:, 1] * s + x, -loc[:, 0] * s + loc[:, 1] * c + y], 1)
    ca, cb = corners(a), corners(b)
    for poly in (ca, cb):
        for k in range(4):
            edge = poly[(k + 1) % 4] - poly[k]
            axis = np.array([-edge[1], edge[0]])
            pa, pb = ca @ axis, cb @ axis
            if pa.max() <= pb.min() or pb.max() <= pa.min():
                return False
    return True


CONTAINMENT = {
    "small inside large": ([0.0, 0.0, 0.0, 4.6, 2.0, 1.6, 0.3], [0.5, 0.2, 0.0, 0.8, 0.6, 1.8, 1.0]),
    "concentric, equal yaw": ([3.0, -2.0, 0.0, 4.0, 2.0, 1.5, 0.7], [3.0, -2.0, 0.0, 2.0, 1.0, 1.5, 0.7]),
    "apart": ([0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0], [6.0, 0.0, 0.0, 1.0, 1.0, 1.5, 0.5]),
    "stand-up boxes overlap, rectangles do not": ([0.0, 0.0, 0.0, 6.0, 1.0, 1.5, 0.785], [2.0, 2.2, 0.0, 1.0, 1.0, 1.5, 0.0]),
    "crossing": ([0.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0], [1.5, 0.8, 0.0, 4.0, 2.0, 1.5, 1.1]),
}


@pytest.mark.parametrize("name", list(CONTAINMENT))
def test_containment_is_a_collision(name):
    a, b = (np.array(v, np.float32) for v in CONTAINMENT[name])
    want = overlap_f64(a[[0, 1, 3, 4, 6]].astype(np.float64), b[[0, 1, 3, 4, 6]].astype(np.float64))
    assert want == (name not in ("apart", "stand-up boxes overlap, rectangles do not"))
    both = np.stack([a, b])
    assert prep.collision_clear(both, both, G.EPS)[0, 1]
    coll = prep.box_collision_test(prep.bev_corners(both), prep.bev_corners(both))
    assert coll.dtype == np.bool_ and coll[0, 1] == want and coll[1, 0] == want, "both ways round"
    assert not coll[0, 0] and not coll[1, 1]
    t = prep.box_collision_test(torch.from_numpy(prep.bev_corners(both)), torch.from_numpy(prep.bev_corners(both)))
    assert torch.is_tensor(t) and t.dtype == torch.bool and np.array_equal(t.numpy(), coll)


def test_a_candidate_inside_a_frame_box_is_rejected():
    frame = np.array([[0.0, 0.0, 0.0, 6.0, 5.0, 2.0, 0.4]], np.float32)
    cand = np.array([[0.3, -0.2, 0.0, 0.8, 0.8, 1.8, 1.0], [20.0, 0.0, 0.0, 0.8, 0.8, 1.8, 1.0]], np.float32)
    assert overlap_f64(frame[0, [0, 1, 3, 4, 6]].astype(np.float64), cand[0, [0, 1, 3, 4, 6]].astype(np.float64))
    assert prep.GTSampler.select_np(frame, cand, [2]).tolist() == [False, True]
    db = {"PEDESTRIAN": [dict(name="PEDESTRIAN", path=str(i), box3d_lidar=cand[i], num_points_in_gt=9, difficulty=0, gt_signs=f"p{i}") for i in (0, 1, 1)]}
    rows = np.arange(45, dtype=np.float32).reshape(9, 5)
    sampler = prep.GTSampler(db, [dict(PEDESTRIAN=2)], points_of=lambda info: rows)
    sampler._samplers["PEDESTRIAN"].indices = np.arange(3)
    got = sampler.sample_all(frame, np.array(["VEHICLE"]), None)
    assert got["gt_names"].tolist() == ["PEDESTRIAN"] and np.array_equal(got["gt_boxes"], cand[1:2]) and got["group_ids"].tolist() == [1]
    assert np.array_equal(got["points"][:, :3], rows[:, :3] + cand[1, :3]) and np.array_equal(got["recon_points"], got["points"])


def test_random_fields_decide_as_the_float64_restatement():
    """every clear pair of a seeded field: crossing or containment in fp32 = the separating-axis answer in float64"""
    inp = G.random_input(3, 40, 40, 1, field=40.0)
    total = np.concatenate([inp["avoid"], inp["cand"]], 0)
    coll = prep.box_collision_test(prep.bev_corners(total), prep.bev_corners(total))
    clear = prep.collision_clear(total, total, G.EPS)
    r = total[:, [0, 1, 3, 4, 6]].astype(np.float64)
    hits = 0
    for i in range(len(total)):
        for j in range(len(total)):
            if i != j and clear[i, j]:
                assert coll[i, j] == overlap_f64(r[i], r[j]), (i, j)
                hits += coll[i, j]
    assert hits >= 20 and clear.mean() > 0.99


# ---- BatchSampler ---------------------------------------------------------------------------------------------------------------------
def test_batch_sampler_edges():
    np.random.seed(3)
    want = np.arange(5); np.random.shuffle(want); first = want.copy()
    np.random.shuffle(want)
    np.random.seed(3)
    s = prep._BatchSampler(5)
    assert np.array_equal(s.sample(9), first) and s.idx == 0 and np.array_equal(s.indices, want)       # num larger than the class: all of it, reshuffled
    a = s.sample(2)
    assert np.array_equal(a, want[:2]) and s.idx == 2
    state = np.random.get_state()[2]
    b = s.sample(3)                                                                                          # the exact fit: the tail, and a reset
    assert np.array_equal(b, want[2:]) and s.idx == 0 and np.random.get_state()[2] != state
    np.random.seed(4)
    s = prep._BatchSampler(6)
    s.sample(4)
    assert len(s.sample(4)) == 2 and s.idx == 0                                                              # a short draw


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    info = dict(name="VEHICLE", path="a", box3d_lidar=np.ones(7, np.float32), num_points_in_gt=9, difficulty=0, gt_signs="a")
    db = {"VEHICLE": [info, info], "PEDESTRIAN": []}
    rows = lambda i: np.zeros((4, 5), np.float32)
    with pytest.raises(NotImplementedError, match="group sampling"):
        prep.GTSampler(db, [dict(VEHICLE=3, PEDESTRIAN=2)], points_of=rows)
    with pytest.raises(NotImplementedError, match="rotation"):
        prep.GTSampler(db, [dict(VEHICLE=3)], points_of=rows, global_rot_range=[-0.5, 0.5])
    with pytest.raises(NotImplementedError, match="rotation"):
        prep.GTSampler(db, [dict(VEHICLE=3)], points_of=rows, global_rot_range=0.3)
    prep.GTSampler(db, [dict(VEHICLE=3)], points_of=rows, global_rot_range=[0, 0.0005])
    sampler = prep.GTSampler(db, [dict(VEHICLE=3), dict(PEDESTRIAN=2)], points_of=rows)
    with pytest.raises(NotImplementedError, match="random_crop"):
        sampler.sample_all(np.zeros((0, 7), np.float32), np.array([]), None, random_crop=True)
    with pytest.raises(_lib.S2DError, match="no database entries"):
        sampler.sample_all(np.zeros((0, 7), np.float32), np.array([]), None)
    with pytest.raises(_lib.S2DError, match="gt_names"):
        prep.GTSampler(db, [dict(VEHICLE=3)], points_of=rows).sample_all(np.zeros((2, 7), np.float32), np.array(["VEHICLE"]), None)
    with pytest.raises(_lib.S2DError, match="columns"):
        prep.GTSampler(db, [dict(VEHICLE=3)], points_of=rows).sample_all(np.ones((1, 9), np.float32), np.array(["CYCLIST"]), None)
    with pytest.raises(_lib.S2DError, match="points_of"):
        prep.GTSampler(db, [dict(VEHICLE=3)])
    with pytest.raises(_lib.S2DError):
        prep.box_collision_test(np.zeros((3, 4, 3), np.float32), np.zeros((3, 4, 2), np.float32))
    with pytest.raises(ValueError):
        prep.GTSampler(db, [dict(VEHICLE=3)], points_of=rows, db_prep_steps=[dict(filter_by_colour=1)])
    with pytest.raises(NotImplementedError, match="db_sampler argument"):
        prep.S2DPreprocess(dict(mode="train", class_names=["VEHICLE"], db_sampler=dict(type="GT-AUG")))
    step = prep.S2DPreprocess(dict(mode="train", class_names=["VEHICLE"], db_sampler=dict(type="GT-AUG")), db_sampler=sampler)
    assert step.db_sampler is sampler
    assert (prep.SAMPLER_LAUNCHES, prep.SAMPLER_HOST_READS, prep.MAX_CANDIDATES, prep.MAX_GROUPS) == (4, 1, 128, 16)


def test_build_gt_sampler_reads_the_reference_dictionary(golden, tmp_path):
    import pickle
    db, rows, _ = G.database(golden, "n")
    cfg = dict(type="GT-AUG", enable=False, db_info_path=str(tmp_path / "dbinfos.pkl"), sample_groups=G.GROUPS, db_prep_steps=G.PREP_STEPS,
               global_random_rotation_range_per_object=[0, 0], rate=1.0)
    np.random.seed(1)
    a = prep.build_gt_sampler(cfg, db_infos=db, points_of=lambda i: rows[i["path"]])      # the path is not opened
    with open(cfg["db_info_path"], "wb") as f:
        pickle.dump(db, f)
    np.random.seed(1)
    b = prep.build_gt_sampler(cfg, points_of=lambda i: rows[i["path"]])
    assert a.classes == b.classes == ["VEHICLE", "PEDESTRIAN", "CYCLIST"] and a.max_nums == [10, 6, 4]
    assert {k: len(v) for k, v in b.db_infos.items()} == {"VEHICLE": 40, "PEDESTRIAN": 8, "CYCLIST": 7}
    assert all(np.array_equal(a._samplers[k].indices, b._samplers[k].indices) for k in a._samplers)
    with pytest.raises(NotImplementedError):
        prep.build_gt_sampler(dict(cfg, global_random_rotation_range_per_object=[-0.3, 0.3]), db_infos=db, points_of=lambda i: rows[i["path"]])


def test_c_entries_validate_before_any_hip_call(lib):
    bad = _lib.S2D_ERR_INVALID_ARG if hasattr(_lib, "S2D_ERR_INVALID_ARG") else -1
    one = ctypes.c_void_p(256)   # never dereferenced: every call below returns from its argument checks
    ends = lambda *v: (ctypes.c_int32 * len(v))(*v)
    assert lib.s2d_prep_gt_scratch_bytes(384, 128) >= 128 * (10 + 4 + 6) * 4
    assert lib.s2d_prep_gt_scratch_bytes(385, 128) == 0 and lib.s2d_prep_gt_scratch_bytes(0, 129) == 0
    assert lib.s2d_prep_gt_scratch_bytes(10, 0) == 0 and lib.s2d_prep_gt_scratch_bytes(-1, 4) == 0
    select = lambda m, s, groups, n_groups, boxes=one, header=one, box_dim=7: lib.s2d_prep_gt_select(
        boxes, m, s, box_dim, groups, n_groups, one, None, 100, 0, 5, one, 1 << 20, header, None)
    paste = lambda s, points_out=one, n=5: lib.s2d_prep_gt_paste(s, 5, one, one, 100, None, 0, one, 1 << 20, one, points_out, None, n, None, 0, None)
    calls = {
        "at most 512 boxes": lambda: select(385, 128, ends(128), 1),
        "129 candidates": lambda: select(10, 129, ends(129), 1),
        "17 groups": lambda: select(10, 20, ends(*range(1, 18)), 17),
        "group ends": lambda: select(10, 20, ends(12, 8), 2),
        "box_dim": lambda: select(10, 20, ends(20), 1, box_dim=6),
        "null boxes": lambda: select(10, 20, ends(20), 1, header=None),
        "prep_gt_paste: 129 candidates": lambda: paste(129),
        "null output": lambda: paste(4, points_out=None),
        "output rows": lambda: paste(4, n=-1),
        "null corners": lambda: lib.s2d_prep_box_collision(one, 4, one, 4, None, None),
        "2^24 pairs": lambda: lib.s2d_prep_box_collision(one, 1 << 13, one, 1 << 12, one, None),
    }
    for text, call in calls.items():
        assert call() == bad, text
        assert text in _lib.last_error(), (text, _lib.last_error())
    assert select(383, 129, ends(129), 1) == bad and "129 candidates" in _lib.last_error()     # M + S = 512 with S = 129
    assert select(385, 128, ends(128), 1) == bad                                                 # M + S = 513
    # a workspace that is too small is reported, not used
    assert lib.s2d_prep_gt_select(one, 10, 20, 7, ends(20), 1, one, None, 100, 0, 5, one, 16, one, None) == -4 and "workspace" in _lib.last_error()
    assert lib.s2d_prep_gt_paste(20, 5, one, one, 100, None, 0, one, 16, one, one, None, 5, None, 0, None) == -4
    # an empty collision matrix is fine without a device
    assert lib.s2d_prep_box_collision(None, 0, None, 5, None, None) == 0


def test_the_device_limits_raise_without_a_device():
    inp = G.random_input(1, 385, 128, 1)
    sampler, store = G.sampler_of(inp)
    with pytest.raises(_lib.S2DError, match="at most 512 boxes"):
        sampler._run_device(inp["avoid"], [(f"G0", i, sampler.db_infos["G0"][i]) for i in range(128)], inp["cand"], inp["ends"], store.get,
                            torch.device("cuda:0"), None, True)


def test_shim_paths_resolve(golden):
    import sparse2dense_amd.det3d_shim as shim
    shim.install()
    from det3d.builder import build_dbsampler
    from det3d.core.bbox.box_np_ops import center_to_corner_box2d
    from det3d.core.sampler.preprocess import box_collision_test
    from det3d.core.sampler.sample_ops import DataBaseSamplerV2
    assert box_collision_test is prep.box_collision_test and build_dbsampler is prep.build_gt_sampler
    b = golden["n_frame_boxes"]
    assert np.array_equal(center_to_corner_box2d(b[:, 0:2], b[:, 3:5], b[:, -1]), prep.bev_corners(b))
    db, rows, _ = G.database(golden, "n")
    np.random.seed(int(golden["seed"]))
    steps = lambda infos: prep._db_filter(prep._db_filter(infos, G.PREP_STEPS[0]), G.PREP_STEPS[1])
    s = DataBaseSamplerV2(db, G.GROUPS, steps, 1.0, [0, 0], points_of=lambda i: rows[i["path"]])   # the reference's positional order
    assert isinstance(s, prep.GTSampler) and len(s.db_infos["VEHICLE"]) == 40 and s.rate == 1.0
