"""Frame preparation without a GPU: the numpy restatement of sparse2dense_amd/prep.py against the golden of the reference's own
`Preprocess.__call__`, `box_np_ops` and `core/sampler/preprocess.py` (tests/golden/frame_prep.npz), the host draws, and the argument
validation of the new C entries (which return before any HIP call).  Criteria: tests/frame_prep_util.py."""
import ctypes

import numpy as np
import pytest
import torch

import frame_prep_util as U
from sparse2dense_amd import _lib, build, prep


@pytest.fixture(scope="module")
def golden(golden_dir):
    return U.load_golden(golden_dir)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("tag", U.CASES)
def test_inside_restatement_equals_the_reference(golden, tag):
    pts, boxes = golden[f"{tag}_points"], golden[f"{tag}_boxes"]
    mask = prep.points_in_rbbox(pts, boxes)
    assert isinstance(mask, np.ndarray) and mask.dtype == np.bool_
    assert np.array_equal(mask, golden[f"{tag}_mask"])
    counts = prep.points_count_rbbox(pts, boxes)
    assert counts.dtype == np.int32 and np.array_equal(counts, golden[f"{tag}_counts"])
    assert golden[f"{tag}_mask"].any() and np.abs(prep.face_distance(pts, boxes)).min() >= U.NEAR_FACE
    # CPU tensors in, tensors out
    tmask = prep.points_in_rbbox(torch.from_numpy(pts), torch.from_numpy(boxes))
    assert torch.is_tensor(tmask) and tmask.dtype == torch.bool and np.array_equal(tmask.numpy(), mask)


@pytest.mark.parametrize("tag", U.CASES)
def test_composition_restatement_equals_the_reference(golden, tag):
    g = golden
    dense, recon = prep.compose_clouds(g[f"{tag}_points"], g[f"{tag}_boxes"], prep.kinds_of(g[f"{tag}_names"]), g[f"{tag}_obj_points"],
                                       g[f"{tag}_obj_offsets"])
    U.check_cloud(dense, g[f"{tag}_comp_dense_points"], f"{tag} dense")
    U.check_cloud(recon, g[f"{tag}_comp_reconstruction_points"], f"{tag} reconstruction")


def test_the_golden_holds_what_it_must(golden):
    g = golden
    mask, kinds, off = g["a_mask"], prep.kinds_of(g["a_names"]), g["a_obj_offsets"]
    assert (mask[:, 0] & mask[:, 1]).sum() >= 3 and off[1] == off[0] and off[2] == off[1]             # overlap of two frame-sourced boxes
    assert (kinds == prep.KIND_SIGN).sum() == 2 and off[7] > off[6]                                    # a SIGN, with a stored cloud to ignore
    y = lambda j: g["a_obj_points"][off[j]:off[j + 1], 1]
    assert (y(2) > 0).sum() > (y(2) < 0).sum() > 0 and 0 < (y(3) > 0).sum() < (y(3) < 0).sum()
    assert (y(4) > 0).sum() == (y(4) < 0).sum() > 0 and (y(4) == 0).sum() > 0                          # the tie, with y == 0 rows
    assert g["a_boxes"].shape == (12, 9) and g["b_boxes"].shape == (12, 7)
    assert g["c_comp_reconstruction_points"].shape == (1, 5) and not g["c_comp_reconstruction_points"].any()
    stored_rows = sum(2 * max((y(j) > 0).sum(), (y(j) < 0).sum()) if kinds[j] == 1 else off[j + 1] - off[j] for j in range(12)
                      if kinds[j] != 2 and off[j + 1] > off[j])
    frame_rows = sum(mask[:, j].sum() for j in range(12) if kinds[j] != 2 and off[j + 1] == off[j])
    assert len(g["a_comp_reconstruction_points"]) < stored_rows + frame_rows                           # the filter drops rows


@pytest.mark.parametrize("kind", list(U.KINDS))
@pytest.mark.parametrize("tag", U.CASES)
def test_preprocess_restatement_equals_the_reference(golden, tag, kind):
    """every cloud, the boxes, names and classes, and the same np.random state after the call as after the reference's"""
    U.run_case(golden, tag, kind, lambda a: a)


def test_draws_come_in_the_references_order():
    cfg = dict(global_rot_noise=0.3, global_scale_noise=[0.9, 1.1], global_translate_std=[0.5, 0.0, 0.0])
    np.random.seed(5)
    d = prep.draw_global_noise(cfg)
    np.random.seed(5)
    fx = np.random.choice([False, True], replace=False, p=[0.5, 0.5]); fy = np.random.choice([False, True], replace=False, p=[0.5, 0.5])
    rot, scale = np.random.uniform(-0.3, 0.3), np.random.uniform(0.9, 1.1)
    t = [np.random.normal(0, 0.5, 1)[0], np.random.normal(0, 0.0, 1)[0], np.random.normal(0, 0.5, 1)[0]]   # the third std is std[0]
    assert (d["flip_x"], d["flip_y"], d["rot"], d["scale"]) == (bool(fx), bool(fy), rot, scale) and np.array_equal(d["translate"], t)
    after = np.random.get_state()[1].copy(), np.random.get_state()[2]
    np.random.seed(5)
    prep.draw_global_noise(dict(cfg, global_translate_std=0))     # no translate: no normal draws
    assert np.random.get_state()[2] != after[1] or not np.array_equal(np.random.get_state()[1], after[0])
    # permutation(n) = the order shuffle() gives an n-row array, with the same draws
    a = np.arange(50, dtype=np.float32).reshape(25, 2)
    np.random.seed(9); want = a.copy(); np.random.shuffle(want); s1 = np.random.get_state()[2]
    np.random.seed(9); got = prep.shuffle_points(a); s2 = np.random.get_state()[2]
    assert np.array_equal(got, want) and s1 == s2


def test_python_argument_checks():
    pts = np.zeros((4, 5), np.float32)
    with pytest.raises(_lib.S2DError, match="at most 512"):
        prep.points_in_rbbox(pts, np.zeros((513, 7), np.float32))
    with pytest.raises(_lib.S2DError):
        prep.points_in_rbbox(pts, np.zeros((3, 6), np.float32))
    with pytest.raises(_lib.S2DError, match="obj_offsets"):
        prep.compose_clouds(pts, np.ones((2, 7), np.float32), [0, 1], np.zeros((3, 5), np.float32), [0, 2, 2])
    with pytest.raises(_lib.S2DError, match="kinds"):
        prep.compose_clouds(pts, np.ones((2, 7), np.float32), [0], np.zeros((0, 5), np.float32), [0, 0, 0])
    with pytest.raises(NotImplementedError):
        prep.S2DPreprocess(dict(mode="train", class_names=["VEHICLE"], db_sampler=dict(type="GT-AUG")))
    with pytest.raises(NotImplementedError):
        prep.S2DPreprocess(dict(mode="val", distillation=True, db_sampler=None))


def test_c_entries_validate_before_any_hip_call(lib):
    bad = _lib.S2D_ERR_INVALID_ARG if hasattr(_lib, "S2D_ERR_INVALID_ARG") else -1
    one = ctypes.c_void_p(256)   # never dereferenced: every call below returns from its argument checks
    assert lib.s2d_prep_workspace_bytes(150000, 100, 20000) > 150000 // 64 * 101 * 4
    assert lib.s2d_prep_workspace_bytes(10, 513, 0) == 0 and lib.s2d_prep_workspace_bytes(-1, 1, 0) == 0
    calls = {
        "boxes": lambda: lib.s2d_prep_points_in_rbbox(one, 10, 5, one, 513, 7, one, None, one, 1 << 20, None),
        "n_points": lambda: lib.s2d_prep_points_in_rbbox(one, -1, 5, one, 3, 7, one, None, one, 1 << 20, None),
        "columns": lambda: lib.s2d_prep_points_in_rbbox(one, 10, 2, one, 3, 7, one, None, one, 1 << 20, None),
        "box_dim": lambda: lib.s2d_prep_points_in_rbbox(one, 10, 5, one, 3, 6, one, None, one, 1 << 20, None),
        "neither": lambda: lib.s2d_prep_points_in_rbbox(one, 10, 5, one, 3, 7, None, None, one, 1 << 20, None),
        "null totals": lambda: lib.s2d_prep_compose_count(one, 10, 5, one, 3, 7, one, None, 0, None, one, 1 << 20, None, None),
        "stored": lambda: lib.s2d_prep_compose_count(one, 10, 5, one, 3, 7, one, None, 4, None, one, 1 << 20, one, None),
        "null output": lambda: lib.s2d_prep_compose_fill(one, 10, 5, 3, None, 0, one, 1 << 20, None, 5, None, 0, None),
        "output rows": lambda: lib.s2d_prep_compose_fill(one, 10, 5, 3, None, 0, one, 1 << 20, one, -1, one, 0, None),
        "null cloud": lambda: lib.s2d_prep_global_noise(None, 5, None, 0, None, 0, 5, 0, 0, 1.0, 0.0, 1.0, 0, 0.0, 0.0, 0.0, None),
        "point columns": lambda: lib.s2d_prep_global_noise(one, 5, None, 0, None, 0, 2, 0, 0, 1.0, 0.0, 1.0, 0, 0.0, 0.0, 0.0, None),
        "in-place": lambda: lib.s2d_prep_gather_rows(one, 5, 5, one, one, None),
    }
    for text, call in calls.items():
        assert call() == bad, text
        assert text in _lib.last_error(), (text, _lib.last_error())
    # a workspace that is too small is reported, not used
    assert lib.s2d_prep_points_in_rbbox(one, 10, 5, one, 3, 7, one, None, one, 16, None) == -4 and "workspace" in _lib.last_error()
    assert lib.s2d_prep_compose_count(one, 10, 5, one, 3, 7, one, None, 0, None, one, 16, one, None) == -4
    # empty calls are fine without a device
    assert lib.s2d_prep_global_noise(None, 0, None, 0, None, 0, 5, 1, 1, 1.0, 0.0, 1.0, 0, 0.0, 0.0, 0.0, None) == 0
    assert lib.s2d_prep_gather_rows(None, 0, 5, None, None, None) == 0
    assert lib.s2d_prep_points_in_rbbox(None, 0, 5, None, 0, 7, one, None, None, 0, None) == 0


def test_shim_exposes_the_inside_test(golden):
    import sparse2dense_amd.det3d_shim as shim
    shim.install()
    from det3d.core.bbox import box_np_ops
    from det3d.datasets.pipelines.preprocess import Preprocess
    assert np.array_equal(box_np_ops.points_in_rbbox(golden["a_points"], golden["a_boxes"]), golden["a_mask"])
    assert np.array_equal(box_np_ops.points_count_rbbox(golden["a_points"], golden["a_boxes"]), golden["a_counts"])
    assert Preprocess is prep.S2DPreprocess
