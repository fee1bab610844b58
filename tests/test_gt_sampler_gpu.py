"""The GT-database sampler on the device (csrc/prep.hip, csrc/box_collision.h through sparse2dense_amd/prep.py): against the golden of the
reference's own `DataBaseSamplerV2` and `Preprocess.__call__` with the criteria of the CPU tests, with per-frame and resident stores, and
against the numpy restatement on seeded random inputs at the sizes where the kernels change path (word edges of the alive mask, the limits
of 512 boxes, 128 candidates and 16 groups, objects longer than a 256-row tile, empty objects and empty blocks).

Condition, not measurement: NO pair the selection can evaluate may be unclear (`collision_clear` at 2e-3 m, cap 0 - one flipped decision
changes every later one).  The seeds below were found with the restatement alone; the test asserts the condition before it compares.
Decisions and row order are exact, the sampled coordinates bit-equal (one fp32 add), the reconstruction coordinates within COORD_ATOL."""
import numpy as np
import pytest
import torch

import frame_prep_util as U
import gt_sampler_util as G
from sparse2dense_amd import _lib, prep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STORES = {"per-frame": None, "resident rows": (DEV, False), "resident": (DEV, True)}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return G.load_golden(golden_dir)


@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("case", ["1", "2", "3", "4", "5"])
def test_device_preprocess_equals_the_reference(golden, case, store):
    G.run_case(golden, case, cuda, resident=STORES[store])


@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("case", ["1", "2"])
def test_device_sample_all_equals_the_reference(golden, case, store):
    sampler, objects, f = G.build_sampler(golden, case, STORES[store], cuda)
    boxes, names = G.kept(f)
    got = sampler.sample_all(boxes, names, objects.get, device=DEV)
    assert np.array_equal(G.rng_words(), golden[f"c{case}_sample_rng"])
    assert got["points"].is_cuda and got["recon_points"].is_cuda
    G.check_sample(got, golden, f"c{case}_sample_")


def test_device_collision_matrix_equals_the_restatement(golden):
    inp = G.random_input(3, 40, 40, 1, field=40.0)
    total = np.concatenate([inp["avoid"], inp["cand"], golden["n_frame_boxes"][:, [0, 1, 2, 3, 4, 5, 8]]], 0)
    corners = prep.bev_corners(total)
    want = prep.box_collision_test(corners, corners[:50])
    got = prep.box_collision_test(cuda(corners), cuda(corners[:50]))
    assert got.is_cuda and got.dtype == torch.bool and got.shape == (len(total), 50)
    clear = prep.collision_clear(total, total[:50], G.EPS)
    assert np.array_equal(got.cpu().numpy()[clear], want[clear]) and want.sum() >= 20 and clear.mean() > 0.99
    assert prep.box_collision_test(cuda(corners[:0]), cuda(corners)).shape == (0, len(total))


# (m, s) -> seed with no unclear pair, found with the restatement alone.  Seed 1 has none at any of the thirty sizes below (on a 150 m field
# with boxes of at most 5 m an unclear pair at 2e-3 m is rare), so the table is empty; the crowded special frame needed seed 4.
SEEDS = {}
M_SIZES, S_SIZES = (0, 1, 63, 64, 65, 384), (1, 2, 64, 65, 128)


def groups_of(m, s):
    return 1 if s < 3 else (3, 16, 1)[(M_SIZES.index(m) + S_SIZES.index(s)) % 3]


def columns_of(m, s):
    return 5 + (M_SIZES.index(m) + S_SIZES.index(s)) % 2


def run(inp, device):
    sampler, store = G.sampler_of(inp)
    return sampler.sample_all(inp["avoid"], np.array(["FRAME"] * len(inp["avoid"])), store.get, device=device)


def compare_with_restatement(inp):
    assert G.unclear_pairs(inp) == 0, "an evaluated pair is unclear: pick another seed"
    want, got, again = run(inp, None), run(inp, DEV), run(inp, DEV)
    accept = prep.GTSampler.select_np(inp["avoid"], inp["cand"], inp["ends"])
    print(f"M {len(inp['avoid'])} S {len(inp['cand'])} groups {len(inp['ends'])}: accepted {int(accept.sum())}")
    if want is None:
        assert got is None and again is None and not accept.any()
        return accept, None
    assert got is not None and np.array_equal(got["gt_boxes"], inp["cand"][accept]) and np.array_equal(want["gt_boxes"], got["gt_boxes"])
    assert got["gt_names"].tolist() == want["gt_names"].tolist() and np.array_equal(got["group_ids"], want["group_ids"])
    assert got["points"].is_cuda and got["points"].dtype == torch.float32
    assert np.array_equal(got["points"].cpu().numpy(), want["points"]), "sampled rows: one fp32 add, the same bits"
    U.check_cloud(got["recon_points"], want["recon_points"], "reconstruction block")
    assert torch.equal(got["points"], again["points"]) and torch.equal(got["recon_points"], again["recon_points"]), "two calls differ"
    return accept, want


@pytest.mark.parametrize("s", S_SIZES)
@pytest.mark.parametrize("m", M_SIZES)
def test_device_equals_the_restatement_at_the_edge_sizes(m, s):
    """M in {0, 1, 63, 64, 65, 384} x S in {1, 2, 64, 65, 128}: 1, 3 and 16 groups, 5 and 6 point columns, M + S = 512 at (384, 128)"""
    compare_with_restatement(G.random_input(SEEDS.get((m, s), 1), m, s, groups_of(m, s), ncols=columns_of(m, s)))


def test_the_edge_sizes_cover_what_they_must():
    shapes = [(m, s) for m in M_SIZES for s in S_SIZES]
    assert {groups_of(*x) for x in shapes} == {1, 3, 16} and {columns_of(*x) for x in shapes} == {5, 6}
    assert (384, 128) in shapes and groups_of(384, 128) > 1


def test_a_chain_of_128_leaves_the_last_one():
    """every candidate crosses its successor: each is rejected because of the next, not yet visited one; the alive mask spans two words"""
    inp = G.random_input(1, 0, 128, 1, chain=True)
    coll = prep.box_collision_test(prep.bev_corners(inp["cand"]), prep.bev_corners(inp["cand"]))
    assert all(coll[i, i + 1] and coll[i + 1, i] for i in range(127)) and coll.sum() == 2 * 127
    accept, want = compare_with_restatement(inp)
    assert accept.tolist() == [False] * 127 + [True]
    inp = G.random_input(1, 70, 128, 1, chain=True)       # the same behind 70 frame boxes: the candidates' bits straddle words 1 to 3
    accept, _ = compare_with_restatement(inp)
    assert accept.tolist() == [False] * 127 + [True]


NOTHING_SEED, EVERYTHING_SEED, LONG_SEED = 4, 1, 1


def test_nothing_accepted_returns_none():
    accept, want = compare_with_restatement(G.random_input(NOTHING_SEED, 20, 40, 3, crowd="all"))
    assert want is None


def test_everything_accepted():
    accept, want = compare_with_restatement(G.random_input(EVERYTHING_SEED, 30, 100, 3, crowd="none"))
    assert accept.all() and len(want["gt_boxes"]) == 100


def test_empty_and_long_objects():
    """an object of 0 rows, one of 257 and one of 700 (more than a 256-row tile) with completed clouds as long, a completed cloud filtered to
    empty; the boxes on a grid, so all are accepted"""
    inp = G.random_input(LONG_SEED, 4, 12, 3, crowd="none")
    rs = np.random.RandomState(5)

    def rows(k, i, cloud):
        b = inp["cand"][i].astype(np.float64)
        half = b[[4, 3, 5]] / 2 if cloud else b[3:6] / 2
        g = np.concatenate([rs.uniform(-1, 1, (k, 3)) * half * (1.3 if cloud else 1.0), rs.uniform(0.01, 1, (k, 2))], 1).astype(np.float32)
        return G.away_from_faces(g, inp["cand"][i]) if cloud else g
    inp["src"][0], inp["cc"][0] = rows(0, 0, False), None
    inp["src"][1], inp["cc"][1] = rows(0, 1, False), rows(90, 1, True)
    inp["src"][2], inp["cc"][2], inp["kinds"][2] = rows(257, 2, False), rows(700, 2, True), 1
    inp["src"][3], inp["cc"][3], inp["kinds"][3] = rows(700, 3, False), rows(300, 3, True), 0
    inp["src"][4], inp["cc"][4] = rows(300, 4, False), None
    far = rows(40, 5, True)
    far[:, 2] += 30.0
    inp["cc"][5] = far
    accept, want = compare_with_restatement(inp)
    assert accept.all() and len(inp["cc"][2]) > 512 and len(inp["cc"][3]) > 256
    sizes = [len(r) for r in inp["src"]]
    assert len(want["points"]) == sum(sizes) and len(want["recon_points"]) < sum(len(c) if c is not None else n for c, n in zip(inp["cc"], sizes))


def test_the_limits_raise():
    for m, s, groups, text in ((385, 128, 1, "at most 512 boxes"), (10, 129, 1, "128"), (10, 40, 17, "16 groups")):
        inp = G.random_input(1, m, s, groups)
        with pytest.raises(_lib.S2DError, match=text):
            run(inp, DEV)


def test_the_scratch_is_guarded_and_written_before_read(monkeypatch):
    """the new entries under poisoned, guard-banded scratch (tests/ws_guard.py): the same bits under both poisons as without"""
    from test_workspace_discipline_gpu import discipline
    inp = G.random_input(1, 65, 65, 3)

    def once():
        got = run(inp, DEV)
        corners = cuda(prep.bev_corners(inp["cand"]))
        return {"points": got["points"], "recon": got["recon_points"], "boxes": cuda(got["gt_boxes"]), "matrix": prep.box_collision_test(corners, corners)}
    discipline(monkeypatch, once, {"prep"})


def test_launch_and_read_budget(golden, monkeypatch):
    """at most 4 launches for the sampler step and one host read (the header); counted at the C entries and at Tensor.tolist"""
    sampler, objects, f = G.build_sampler(golden, "1", (DEV, True), cuda)
    boxes, names = G.kept(f)
    lib = _lib.load()
    calls, reads = [], []
    launches = {"s2d_prep_gt_select": 3, "s2d_prep_gt_paste": 1}

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name.startswith("s2d_prep_") and name != "s2d_prep_gt_scratch_bytes":
                def wrapped(*a):
                    calls.append(name)
                    return fn(*a)
                return wrapped
            return fn
    monkeypatch.setattr(_lib, "load", lambda: Counting())
    tolist = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: (reads.append(tuple(t.shape)), tolist(t))[1])
    got = sampler.sample_all(boxes, names, objects.get, device=DEV)
    assert got is not None and sorted(calls) == ["s2d_prep_gt_paste", "s2d_prep_gt_select"]
    assert sum(launches[c] for c in calls) == prep.SAMPLER_LAUNCHES <= 4 and reads == [(2 + 11,)] and prep.SAMPLER_HOST_READS == 1


def test_prepared_frames_with_a_sampler_feed_a_student_step():
    """PreparedFrames(db_sampler=...) at 12 k points: pasted objects reach the boxes and the clouds, one student step has a finite loss and
    finite gradients"""
    from sparse2dense_amd import scene, waymo_configs
    from sparse2dense_amd.data import PreparedFrames
    from sparse2dense_amd.registry import build_detector
    s = scene.make_scene(12000, seed=7)
    names = [scene.WAYMO_CLASS_NAMES[c - 1] for c in s["gt_classes"]]
    frames = [dict(points=s["points"], gt_boxes=s["gt_boxes"], gt_names=names, objects=scene.make_object_clouds(s, seed=11, n_total=2000))]
    rs = np.random.RandomState(3)
    db, rows = {}, {}
    for name, size in (("VEHICLE", (4.5, 2.0, 1.6)), ("PEDESTRIAN", (0.8, 0.8, 1.8)), ("CYCLIST", (1.8, 0.8, 1.7))):
        db[name] = []
        for k in range(20):
            box = np.concatenate([rs.uniform(-60, 60, 2), [0.0], size, rs.normal(0, 2, 2), rs.uniform(-3, 3, 1)]).astype(np.float32)
            n = int(rs.randint(20, 80))
            rows[f"{name}{k}"] = np.concatenate([rs.uniform(-1, 1, (n, 3)) * box[3:6] / 2, rs.uniform(0, 1, (n, 2))], 1).astype(np.float32)
            db[name].append(dict(name=name, path=f"{name}{k}", box3d_lidar=box, num_points_in_gt=n, difficulty=0, gt_signs=f"db_{name}{k}"))
    np.random.seed(0)
    count = lambda n: sum(x == n for x in names)
    sampler = prep.GTSampler(db, [{n: count(n) + 6} for n in scene.WAYMO_CLASS_NAMES], points_of=lambda i: rows[i["path"]]).resident(DEV)
    source = PreparedFrames(frames, device=DEV, db_sampler=sampler)
    ex = source.example()
    plain = PreparedFrames(frames, device=DEV)
    plain.prepare()
    added = source.points[0].shape[0] - plain.points[0].shape[0]
    assert added > 0 and source.dense_points[0].shape[0] - plain.dense_points[0].shape[0] == added
    assert source.recon_points[0].shape[0] - plain.recon_points[0].shape[0] == added        # no completed clouds for the database: the rows themselves
    assert int((source.gt_classes[0] > 0).sum()) > len(names)
    torch.manual_seed(0)
    student = build_detector(waymo_configs.s2d_student()).to(DEV).train()
    losses, _, _, _, mask_loss, offset_loss = student(ex, return_loss=True, return_feature=True)
    loss = sum(losses["loss"]) + mask_loss + offset_loss
    assert torch.isfinite(loss).item()
    loss.backward()
    grads = [p.grad for p in student.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all().item() for g in grads)
