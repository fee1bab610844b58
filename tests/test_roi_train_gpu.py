"""The RoI head's training branch on the kernels of csrc/roi_mlp_train.hip (second_stage.roi_mlp_train_fused, roi_loss_fused,
RoIHead.fused_training) against the float64 definitions, the reference's recorded training step and the torch chain it replaces.

Parity rule (test_roi_mlp_gpu.py's): with e_chain the largest absolute error of the fp32 torch chain - the module's own layers with the SAME
dropout masks, the head's own loss functions, autograd - against the float64 definition and e_fused that of the kernels,
e_fused <= 4 e_chain + 1e-7 max|ref| for every compared tensor; tensors of fewer than 256 elements are divided by their max|ref| and pooled
(roi_train_util.check_step).  The seeds are chosen in test_roi_train_cpu.py so that the rule's conditions hold."""
import copy
import os

import numpy as np
import pytest
import torch

from golden_util import fill_params, seeded
from roi_train_util import LOSS_CFG, SHAPES, TWO_ROWS, check_pool, check_step, collect, draw_masks, layers_of, make_case, make_train_head, run_step
from sparse2dense_amd import registry, second_stage as S
from test_second_stage import ROI_TRAIN_CFG, _check_roi_training

pytestmark = pytest.mark.gpu


def test_golden_training_step_through_the_fused_path(golden_dir):
    """roi_training.npz through RoIHead.forward(training=True, device=True) with fused_training set, get_loss() and backward(): the set-up,
    seeds and tolerances of test_roi_device_gpu.test_roi_head_training_branch_on_the_device_path_matches_the_reference.  Logits of 219."""
    g = np.load(os.path.join(golden_dir, "roi_training.npz"))
    roi = registry.build(dict(type="RoIHead", input_channels=40, code_size=7, model_cfg=ROI_TRAIN_CFG), registry.ROI_HEAD)
    fill_params(roi).train().to("cuda")
    roi.fused_training = True
    np.random.seed(int(g["np_seed"])); torch.manual_seed(int(g["torch_seed"]))
    t = lambda k: torch.from_numpy(g[k]).cuda()
    batch = dict(rois=t("rois"), roi_labels=t("roi_labels"), roi_scores=t("roi_scores"), roi_features=t("roi_features"), gt_boxes_and_cls=t("gt"))
    roi(batch, training=True, device=True)
    assert roi.train_reason is None and roi.train_paths == {"fused": 1, "torch": 0} and roi.mlp_paths == {"fused": 0, "torch": 0}
    total, tb = roi.get_loss()
    assert isinstance(tb["rcnn_loss"], float) and total.grad_fn is not None
    total.backward()
    ret = roi.forward_ret_dict
    _check_roi_training(g, roi, ret, total, tb, rtol=2e-4, atol=2e-5)
    assert ret["rcnn_cls"].shape == (64, 1) and ret["rcnn_reg"].shape == (64, 7) and float(ret["rcnn_cls"].detach().abs().max()) > 200
    assert all(int(bn.num_batches_tracked) == 1 for _, bn in layers_of(roi) if bn is not None)


@pytest.mark.parametrize("shape", SHAPES + [TWO_ROWS], ids=lambda s: f"cin{s[0]}-rows{s[4]}")
def test_kernels_agree_with_the_float64_definition_like_the_torch_chain_does(shape):
    """outputs, both losses, every weight / gamma / beta / bias gradient, the running statistics and num_batches_tracked, with p = 0.3
    masks.  Two rows: x_hat = +-1, the norm's data gradient is a difference of equal numbers in both implementations, so only the forward,
    the statistics, the losses and the final layers' gradients are compared."""
    cin, shared, cls, reg, rows, seed = shape
    head = make_train_head(cin, shared, cls, reg, seed=seed).cuda()
    case, masks = make_case(cin, rows, seed), draw_masks(head, rows, 31 + seed)
    ref, chain, got = (run_step(head, case, masks, how) for how in ("ref", "chain", "fused"))
    assert all(l["tracked"] == 1 for l in got["layers"] if "tracked" in l)
    check_step(ref, chain, got, data_grads=rows > 2)


def test_eval_kernel_follows_the_statistics_the_training_kernels_moved():
    """the running statistics are written through raw pointers; num_batches_tracked is bumped by an ordinary in-place add, whose version
    the eval kernel's cached scale / shift vector is keyed on"""
    head = make_train_head(40, (64, 64), (64, 64), (64, 64)).cuda()
    x = seeded((21, 40), 13).cuda()
    with torch.no_grad():
        before = S.roi_mlp_fused(head.eval(), x)
    affine = head._mlp_cache["affine"]
    S.roi_mlp_train_fused(head.train(), seeded((33, 40), 14).cuda() * 2 + 1)
    with torch.no_grad():
        after = S.roi_mlp_fused(head.eval(), x)
        ref = S.roi_mlp_reference(copy.deepcopy(head).double(), x.double())
    assert head._mlp_cache["affine"] is not affine
    for a, b, r in zip(before, after, ref):
        assert float((a - b).abs().max()) > 1e-3
        np.testing.assert_allclose(b.cpu().numpy(), r.cpu().numpy(), rtol=1e-4, atol=1e-5)


def _step(head, case, masks):
    """(rcnn_cls, rcnn_reg, loss_cls, loss_reg, gradients) of one fused step on a copy of the head"""
    head = copy.deepcopy(head)
    cls, reg = S.roi_mlp_train_fused(head, case["x"].cuda(), masks)
    losses = S.roi_loss_fused(cls, reg, case["labels"].cuda(), case["fg"].cuda(), case["target"].cuda(), LOSS_CFG)
    (losses[0] + losses[1]).backward()
    return [cls.detach(), reg.detach(), losses[0].detach(), losses[1].detach()] + [p.grad for p in head.parameters()] + \
           [b for n, b in head.named_buffers() if "running" in n]


def test_ragged_rows_statistics_see_every_row_and_scratch_is_written_before_read(monkeypatch):
    """batch statistics couple the rows: appending rows changes EVERY row's output (R = 17 is not the first 17 rows of R = 20).  A call on
    R = 17 - two tiles, fifteen absent rows - with its scratch pre-filled with NaN is bit-equal to one with zero-filled scratch."""
    head = make_train_head(40, (64, 64), (), (64, 64)).cuda()
    case, masks = make_case(40, 20, 3), draw_masks(head, 20, 5)
    head17 = lambda: {k: v[:17] for k, v in case.items()}
    full = _step(head, case, masks)
    part = _step(head, head17(), [m[:17] for m in masks])
    for a, b in zip(part[:2], full[:2]):
        assert bool(((a - b[:17]).abs() > 0).any(dim=1).all())
    fills, arenas, guard = [], [], 1024

    def scratch(n, dev, value):   # the scratch between two guard bands of -7
        arena = torch.full((n + 2 * guard,), -7.0, dtype=torch.float32, device=dev)
        arena[guard:guard + n] = value
        arenas.append(arena)
        return arena[guard:guard + n]
    for value in (float("nan"), 0.0):
        monkeypatch.setattr(S, "_roi_train_workspace", lambda n, dev, value=value: scratch(n, dev, value))
        fills.append(_step(head, head17(), [m[:17] for m in masks]))
    for a, b, c in zip(*fills, part):
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)
    # neither the forward nor the backward wrote outside the scratch it asked for, and both wrote finite numbers into all they read
    assert len(arenas) == 2 and arenas[0].numel() > 2 * guard + 17 * 64 * 8
    for arena in arenas:
        assert bool((arena[:guard] == -7.0).all()) and bool((arena[-guard:] == -7.0).all())
    assert torch.isfinite(arenas[0][guard:-guard]).all()   # (this shape leaves no word of the NaN-filled scratch unwritten)


def test_same_inputs_same_bits():
    cin, shared, cls, reg, rows, seed = SHAPES[0]
    head = make_train_head(cin, shared, cls, reg).cuda()
    case, masks = make_case(cin, rows, 1), draw_masks(head, rows, 2)
    first, second = _step(head, case, masks), _step(head, case, masks)
    assert len(first) == len(second) == 4 + 22 + 12
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # masks=None draws every site's mask in one call from torch's CUDA generator: the same seed, the same step
    torch.manual_seed(7)
    a = _step(head, case, None)
    torch.manual_seed(7)
    b = _step(head, case, None)
    torch.manual_seed(8)
    c = _step(head, case, None)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[1], c[1]) and not torch.equal(a[1], first[1])


@pytest.mark.parametrize("kind", ["no valid", "no fg", "saturated", "hard"])
def test_loss_kernel_edge_cases(kind):
    """against the definition evaluated by torch in fp32 and float64 on the same predictions; |logit| = 200 gives exactly zero gradient"""
    from test_roi_train_cpu import _loss_case
    cls, reg, labels, fg, target = (t.cuda() for t in _loss_case(kind))
    c, r = cls.float().requires_grad_(), reg.float().requires_grad_()
    lc, lr = S.roi_loss_fused(c, r, labels.reshape(2, 12), fg.reshape(2, 12), target, LOSS_CFG)
    assert lc.shape == lr.shape == () and lc.grad_fn is not None
    (2 * lc + 3 * lr).backward()
    c64, r64 = cls.float().double().requires_grad_(), reg.float().double().requires_grad_()
    lc64, lr64 = S.roi_loss_reference(c64, r64, labels, fg, target.double(), LOSS_CFG)
    (2 * lc64 + 3 * lr64).backward()
    for a, b in [(lc, lc64), (lr, lr64), (c.grad, c64.grad), (r.grad, r64.grad)]:
        assert a.dtype == torch.float32 and a.shape == b.shape
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=2e-6, atol=1e-7)
    if kind == "no valid":
        assert float(lc) == 0 and float(c.grad.abs().max()) == 0 and float(lr) > 0
    if kind == "no fg":
        assert float(lr) == 0 and float(r.grad.abs().max()) == 0 and float(lc) > 0
    if kind == "saturated":
        assert torch.equal(c.grad[3:7], torch.zeros_like(c.grad[3:7])) and float(c.grad.abs().max()) > 0 and float(lc) > 6.25
    if kind == "hard":
        assert float(c.grad[::3].abs().max()) == 0 and float(c.grad[1::3].abs().min()) > 0


def test_head_level_switch_changes_the_path_and_not_the_step(golden_dir):
    """DP_RATIO = 0, the same numpy / torch seeds: fused_training on and off sample the same targets, and both steps' losses and .grad's
    stand to the float64 definitions on those targets as the rule asks"""
    g = np.load(os.path.join(golden_dir, "roi_training.npz"))
    base = make_train_head(40, (64, 64), (64, 64), (64, 64), dp=0.0, TARGET_CONFIG=ROI_TRAIN_CFG["TARGET_CONFIG"]).cuda()
    t = lambda k: torch.from_numpy(g[k]).cuda()
    runs = {}
    for fused in (False, True):
        head = copy.deepcopy(base)
        head.fused_training = fused
        np.random.seed(3); torch.manual_seed(4)
        head(dict(rois=t("rois"), roi_labels=t("roi_labels"), roi_scores=t("roi_scores"), roi_features=t("roi_features"), gt_boxes_and_cls=t("gt")),
             training=True, device=True)
        total, tb = head.get_loss()
        total.backward()
        ret = head.forward_ret_dict
        assert head.train_paths == ({"fused": 1, "torch": 0} if fused else {"fused": 0, "torch": 1}) and bool(ret.get("fused_training")) == fused
        assert head.mlp_paths == {"fused": 0, "torch": 0 if fused else 1}
        np.testing.assert_allclose(tb["rcnn_loss"], float(tb["rcnn_loss_cls"]) + float(tb["rcnn_loss_reg"]), rtol=1e-6)
        runs[fused] = (ret, collect(head, ret["rcnn_cls"], ret["rcnn_reg"], tb["rcnn_loss_cls"], tb["rcnn_loss_reg"]))
    for k in ("rois", "gt_of_rois", "rcnn_cls_labels", "reg_valid_mask", "roi_features", "roi_labels"):
        assert torch.equal(runs[False][0][k], runs[True][0][k]), k
    ret = runs[True][0]
    assert int(ret["reg_valid_mask"].sum()) > 0
    case = dict(x=ret["roi_features"].reshape(-1, 40), labels=ret["rcnn_cls_labels"].reshape(-1), fg=ret["reg_valid_mask"].reshape(-1),
                target=ret["gt_of_rois"].reshape(-1, ret["gt_of_rois"].shape[-1]))
    check_step(run_step(base, case, None, "ref"), runs[False][1], runs[True][1])
