"""The fused eval RoI MLP (csrc/roi_mlp.hip through second_stage.RoIHead) against its float64 definition (second_stage.roi_mlp_reference),
the reference's recorded outputs, and the torch MLP it replaces.

Tolerance rule of the parity checks: with e_chain the largest absolute error of the torch fp32 module against the float64 reference on the
same inputs and e_fused that of the kernel, e_fused <= 4 * e_chain + 1e-7 * max|out|.  Both are fp32 sums over the same products in
different orders; the factor covers the spread between two such orderings over a few thousand outputs, not a lost term or a wrong scale
(1e-3 or more)."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from golden_util import fill_params, seeded
from sparse2dense_amd import _lib, second_stage as S
from test_roi_mlp_cpu import make_head, module_mlp

pytestmark = pytest.mark.gpu


def check_parity(head, x):
    """the tolerance rule above on (rcnn_cls | rcnn_reg) of x [R, cin]; returns the kernel's outputs"""
    ref = torch.cat(S.roi_mlp_reference(copy.deepcopy(head).double(), x.double()), dim=1)
    chain = torch.cat(module_mlp(head, x), dim=1)
    with torch.no_grad():
        cls, reg = S.roi_mlp_fused(head, x)
    assert cls.shape == (x.shape[0], 1) and reg.shape == (x.shape[0], 7) and cls.dtype == reg.dtype == torch.float32
    e_chain = float((chain.double() - ref).abs().max())
    e_fused = float((torch.cat([cls, reg], dim=1).double() - ref).abs().max())
    top = float(ref.abs().max())
    print(f"cin {x.shape[1]}, R {x.shape[0]}: e_chain {e_chain:.3e}, e_fused {e_fused:.3e}, max|out| {top:.3e}")
    assert 1e-2 < top < 1e12
    assert e_fused <= 4 * e_chain + 1e-7 * top, (e_fused, e_chain, top)
    return cls, reg


@pytest.mark.parametrize("cin,shared,cls,reg,rows", [
    (2560, (256, 256), (256, 256), (256, 256), 37),   # the two-stage configs: 20 staged chunks, four accumulators per wave, three row tiles
    (40, (64, 64), (), (64, 64), 17),                 # CLS_FC = []: a cin below one chunk that ends in single steps, one accumulator per wave
    (512, (256,), (256, 256), (256, 256), 16),        # one shared layer: the branches read buffer 0; exactly one row tile
])
def test_kernel_agrees_with_the_float64_reference_like_the_torch_mlp_does(cin, shared, cls, reg, rows):
    head = make_head(cin, shared, cls, reg, signed=True).cuda()
    check_parity(head, seeded((rows, cin), 11).cuda())


def test_golden_fixture_through_the_fused_mlp(golden_dir):
    """(120, 64, 50): cin = 30 steps = three whole groups of 8 and six single steps; 50 slots of which the last 10 are zero padding"""
    g = np.load(os.path.join(golden_dir, "second_stage.npz"))
    head = make_head(120, (64, 64), (64, 64), (64, 64)).cuda()
    rois = torch.zeros(1, 50, 7); rois[0, :40] = torch.from_numpy(g["boxes"])
    feats = torch.zeros(1, 50, 120); feats[0, :40] = torch.from_numpy(g["bev_features"])
    scores = torch.zeros(1, 50); scores[0, :40] = seeded((40,), 31).abs().clamp(max=1.0)
    labels = torch.zeros(1, 50, dtype=torch.long); labels[0, :40] = 1 + torch.arange(40) % 3
    cls, _ = check_parity(head, feats.cuda().view(50, 120))
    np.testing.assert_allclose(cls.view(1, 50, 1).cpu().numpy(), g["batch_cls_preds"], rtol=1e-4, atol=1e-5)
    with torch.no_grad():
        out = head(dict(rois=rois.cuda(), roi_features=feats.cuda(), roi_scores=scores.cuda(), roi_labels=labels.cuda()), training=False, device=True)
    assert head.mlp_paths == {"fused": 1, "torch": 0}
    np.testing.assert_allclose(out["batch_cls_preds"].cpu().numpy(), g["batch_cls_preds"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out["batch_box_preds"].cpu().numpy(), g["batch_box_preds"], rtol=1e-4, atol=1e-5)


@pytest.fixture(scope="module")
def wide():
    """one set of weights (cin 2560, widths 256), 250 rows of which the last 10 are zero, and the kernel's outputs for all of them"""
    head = make_head(2560, (256, 256), (256, 256), (256, 256), signed=True).cuda()
    x = seeded((250, 2560), 12).cuda()
    x[240:] = 0
    with torch.no_grad():
        return head, x, S.roi_mlp_fused(head, x)


@pytest.mark.parametrize("rows", [1, 15, 16, 17])
def test_a_rows_result_does_not_depend_on_the_rest_of_the_call(wide, rows):
    head, x, full = wide
    with torch.no_grad():
        part = S.roi_mlp_fused(head, x[:rows])
    for a, b in zip(part, full):
        assert a.shape[0] == rows and torch.equal(a, b[:rows])


def test_zero_rows_get_the_bits_of_an_all_zero_call(wide):
    head, x, full = wide
    with torch.no_grad():
        zero = S.roi_mlp_fused(head, torch.zeros(1, 2560, device="cuda"))
    for a, b in zip(zero, full):
        assert float(a.abs().max()) > 0 and torch.equal(b[240:], a.expand(10, -1))
        assert not torch.equal(b[239:240], a)


def test_cached_images_follow_the_parameters():
    head = make_head(120, (64, 64), (64, 64), (64, 64)).cuda()
    x = seeded((21, 120), 13).cuda()
    first = check_parity(head, x)
    packed, affine = head._mlp_cache["packed"], head._mlp_cache["affine"]
    check_parity(head, x)
    assert head._mlp_cache["packed"] is packed and head._mlp_cache["affine"] is affine                 # nothing changed: nothing rebuilt
    with torch.no_grad():
        head.shared_fc_layer[0].weight.add_(0.05)
    moved = check_parity(head, x)
    assert head._mlp_cache["packed"] is not packed and head._mlp_cache["affine"] is affine             # a weight: the image only
    assert float((moved[0] - first[0]).abs().max()) > 1e-3
    packed = head._mlp_cache["packed"]
    with torch.no_grad():
        head.cls_layers[1].running_mean.add_(0.3)
    again = check_parity(head, x)
    assert head._mlp_cache["packed"] is packed and head._mlp_cache["affine"] is not affine             # a running statistic: scale / shift only
    assert float((again[0] - moved[0]).abs().max()) > 1e-3 and torch.equal(again[1], moved[1])
    head.load_state_dict(make_head(120, (64, 64), (64, 64), (64, 64), seed=1).state_dict())
    loaded = check_parity(head, x)
    assert float((loaded[1] - again[1]).abs().max()) > 1e-3
    from sparse2dense_amd.dense2d import clear_pack_cache, refresh_pack_cache
    packed = head._mlp_cache["packed"]
    clear_pack_cache()                                                                                 # what checkpoint.load_checkpoint calls
    assert all(torch.equal(a, b) for a, b in zip(check_parity(head, x), loaded)) and head._mlp_cache["packed"] is not packed
    # a training-mode forward moves the running statistics without moving their version counters
    head.train()
    module_mlp(head, seeded((64, 120), 15).cuda() * 2 + 1)
    head.eval()
    trained = check_parity(head, x)
    assert float((trained[0] - loaded[0]).abs().max()) > 1e-3
    # the fused Adam writes the parameters through raw pointers and then calls refresh_pack_cache()
    head.reg_layers[0].weight.data.mul_(1.5)
    refresh_pack_cache()
    assert float((check_parity(head, x)[1] - trained[1]).abs().max()) > 1e-3


@pytest.mark.parametrize("width", [64, 256])
def test_pack_writes_the_b_fragment_order(width):
    """image[w_off + (ks * tiles + t) * 64 + l] = W[16 t + (l & 15)][4 ks + (l >> 4)], rows past cout zero"""
    lib = _lib.load()
    cin = 40
    plan = _lib.RoiMlpPlan()
    _lib.check(lib.s2d_roi_mlp_plan_make(cin, 2, width, width, 1, width, 0, 2, width, width, 1, 7, ctypes.byref(plan)))
    shapes = [(l.cout, l.cin) for l in plan.layer[:plan.num_layers]]
    assert shapes == [(width, cin), (width, width), (width, width), (1, width), (width, width), (width, width), (7, width)]
    weights = [seeded(s, 50 + i).cuda() for i, s in enumerate(shapes)]
    packed = torch.full((plan.packed_elems,), float("nan"), device="cuda")
    ptrs = (ctypes.c_void_p * len(weights))(*[w.data_ptr() for w in weights])
    _lib.check(lib.s2d_roi_mlp_pack(ctypes.byref(plan), ptrs, packed.data_ptr(), torch.cuda.current_stream().cuda_stream), "s2d_roi_mlp_pack")
    got = packed.cpu().numpy()
    for l, w in zip(plan.layer[:plan.num_layers], weights):
        full = np.zeros((l.cout_pad, l.cin), np.float32)
        full[:l.cout] = w.cpu().numpy()
        # [tile t][column c][step ks][k-lane q] -> [ks][t][q][c]: lane = 16 q + c
        want = full.reshape(l.cout_pad // 16, 16, l.cin // 4, 4).transpose(2, 0, 3, 1).reshape(-1)
        assert np.array_equal(got[l.w_off:l.w_off + want.size], want), (l.cin, l.cout)
    assert plan.layer[plan.num_layers - 1].w_off + 16 * width == plan.packed_elems == got.size


def test_detector_inference_runs_the_fused_mlp_and_agrees_with_the_torch_mlp(monkeypatch, golden_dir):
    from sparse2dense_amd import waymo_configs
    from sparse2dense_amd.data import SyntheticFrames
    from test_roi_device_gpu import TEST_CFG, _detector, _replay_first_stage
    from test_second_stage import ROI_TRAIN_CFG
    torch.manual_seed(0)
    det = _detector(waymo_configs.s2d_student(), dict(ROI_TRAIN_CFG, SHARED_FC=[256, 256], CLS_FC=[256, 256], REG_FC=[256, 256], DP_RATIO=0.3)).eval()
    det.single_det.test_cfg = dict(TEST_CFG, score_threshold=0.05)
    ex = SyntheticFrames(2, n_points=20000, seed=5, device="cuda").example()
    _replay_first_stage(det, ex, False)
    head = det.roi_head
    monkeypatch.delenv("S2D_ROI_DEVICE", raising=False)
    monkeypatch.delenv("S2D_ROI_MLP", raising=False)
    with torch.no_grad():
        dev = det(dict(ex), return_loss=False)
        assert head.mlp_paths == {"fused": 1, "torch": 0}
        monkeypatch.setenv("S2D_ROI_MLP", "0")
        ref = det(dict(ex), return_loss=False)
    assert head.mlp_paths == {"fused": 1, "torch": 1} and det.roi_paths == {"device": 2, "torch": 0}
    assert len(dev) == len(ref) == 2
    for d, r in zip(dev, ref):
        assert 0 < len(r["scores"]) <= 500 and d["box3d_lidar"].shape == r["box3d_lidar"].shape and torch.equal(d["label_preds"], r["label_preds"])
        np.testing.assert_allclose(d["box3d_lidar"].cpu().numpy(), r["box3d_lidar"].cpu().numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(d["scores"].cpu().numpy(), r["scores"].cpu().numpy(), rtol=1e-4, atol=1e-6)
    # the training branch keeps the torch MLP (batch statistics, dropout, a backward pass)
    monkeypatch.delenv("S2D_ROI_MLP", raising=False)
    det.train()
    assert head.training and "training mode" in head.mlp_reason(torch.zeros(2, 60, 2560, device="cuda"))
    g = np.load(os.path.join(golden_dir, "roi_training.npz"))
    t = lambda k: torch.from_numpy(g[k]).cuda()
    np.random.seed(int(g["np_seed"])); torch.manual_seed(int(g["torch_seed"]))
    head(dict(rois=t("rois"), roi_labels=t("roi_labels"), roi_scores=t("roi_scores"), roi_features=seeded((2, 60, 2560), 14).cuda(),
              gt_boxes_and_cls=t("gt")), training=True, device=True)
    assert head.mlp_paths == {"fused": 1, "torch": 2} and head.forward_ret_dict["rcnn_reg"].requires_grad
