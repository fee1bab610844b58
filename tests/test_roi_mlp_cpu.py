"""The definition the fused RoI MLP kernel implements (second_stage.roi_mlp_reference) against the module's own layers and the reference's
recorded outputs, the reasons RoIHead.mlp_reason names, and the layer table of csrc/roi_mlp.hip - all without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from golden_util import fill_params, seeded
from sparse2dense_amd import _lib, registry, second_stage as S


def make_head(cin, shared, cls, reg, code_size=7, seed=0, signed=False):
    """fill_params gives a [cout, cin, 1] convolution weight the all-positive values of a norm scale (the golden fixtures were recorded
    that way): no cancellation, outputs of 1e8 and more.  signed=True redraws the convolution weights as N(0, 1.5 / cin), so that the sums
    cancel as a trained head's do and the activations keep their scale from layer to layer."""
    cfg = dict(CLASS_AGNOSTIC=True, SHARED_FC=list(shared), CLS_FC=list(cls), REG_FC=list(reg), DP_RATIO=0.3)
    head = registry.build(dict(type="RoIHead", input_channels=cin, code_size=code_size, model_cfg=cfg), registry.ROI_HEAD)
    fill_params(head, seed)
    if signed:
        with torch.no_grad():
            for i, m in enumerate(m for m in head.modules() if isinstance(m, torch.nn.Conv1d)):
                m.weight.copy_(seeded(m.weight.shape, 1000 + 17 * seed + i, (1.5 / m.in_channels) ** 0.5))
    return head.eval()


def module_mlp(head, x):
    """the three nn.Sequential's as RoIHead.forward runs them: x [R, cin] -> (rcnn_cls [R, 1], rcnn_reg [R, code])"""
    with torch.no_grad():
        shared = head.shared_fc_layer(x.reshape(-1, 1, x.shape[-1]).permute(0, 2, 1).contiguous())
        return (head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1), head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1))


@pytest.mark.parametrize("shared,cls,reg", [((64, 64), (64, 64), (64, 64)), ((64,), (), (48, 32)), ((32, 64), (16,), ())])
def test_reference_is_the_modules_own_eval_forward_in_float64(shared, cls, reg):
    """pins eps, the layer order, the Conv1d weight squeeze and the two final biases: depths (2, 2, 2), (1, 0, 2) and (2, 1, 0)"""
    head = make_head(40, shared, cls, reg, signed=len(shared) == 1).double()
    x = seeded((23, 40), 3).double()
    got, ref = S.roi_mlp_reference(head, x), module_mlp(head, x)
    assert got[0].shape == (23, 1) and got[1].shape == (23, 7) and got[0].dtype == torch.float64
    for a, b in zip(got, ref):
        assert float(b.abs().max()) > 1e-3
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=0)
    # leading dimensions are flattened
    assert torch.equal(S.roi_mlp_reference(head, x[:22].reshape(2, 11, 40))[1], got[1][:22])


def test_reference_reproduces_the_reference_projects_cls_preds(golden_dir):
    """the set-up of test_second_stage.py: cin 120, widths 64, 50 slots of which the last 10 are zero padding"""
    g = np.load(os.path.join(golden_dir, "second_stage.npz"))
    head = make_head(120, (64, 64), (64, 64), (64, 64))
    feats = torch.zeros(1, 50, 120)
    feats[0, :40] = torch.from_numpy(g["bev_features"])
    cls, reg = S.roi_mlp_reference(head, feats)
    assert cls.dtype == torch.float32 and reg.shape == (50, 7)
    np.testing.assert_allclose(cls.view(1, 50, 1).numpy(), g["batch_cls_preds"], rtol=1e-4, atol=1e-5)


def test_mlp_reason_names_what_keeps_the_torch_mlp(monkeypatch):
    monkeypatch.delenv("S2D_ROI_MLP", raising=False)
    x = torch.zeros(4, 40)
    head = make_head(40, (64, 64), (64, 64), (64, 64))
    assert "CPU tensor" in head.mlp_reason(x)
    assert "training mode" in head.train().mlp_reason(x)
    assert "width 200" in make_head(40, (64, 200), (64,), (64,)).mlp_reason(x)
    assert "3 shared layers" in make_head(40, (64, 64, 64), (64,), (64,)).mlp_reason(x)
    assert "code_size 9" in make_head(40, (64,), (64,), (64,), code_size=9).mlp_reason(x)
    assert "42 input channels" in make_head(42, (64,), (), ()).mlp_reason(x)
    monkeypatch.setenv("S2D_ROI_MLP", "0")
    assert head.eval().mlp_reason(x) == "S2D_ROI_MLP=0"
    assert head.mlp_paths == {"fused": 0, "torch": 0}
    with pytest.raises(_lib.S2DError, match="S2D_ROI_MLP=0"):
        S.roi_mlp_fused(head, x)   # the direct entry has no fallback


def test_shape_family_and_layer_table_of_the_library():
    lib = _lib.load()   # loads without a GPU
    ok = lambda *a: lib.s2d_roi_mlp_supported(*a)
    #          cin  shared       cls          reg       classes code
    assert ok(2560, 2, 256, 256, 2, 256, 256, 2, 256, 256, 1, 7) and ok(40, 1, 64, 0, 0, 0, 0, 2, 48, 32, 1, 7) and ok(4096, 2, 16, 16, 1, 16, 0, 0, 0, 0, 1, 7)
    for bad in [(42, 1, 64, 0, 0, 0, 0, 0, 0, 0, 1, 7), (4100, 1, 64, 0, 0, 0, 0, 0, 0, 0, 1, 7), (40, 3, 64, 64, 0, 0, 0, 0, 0, 0, 1, 7),
                (40, 0, 0, 0, 1, 64, 0, 1, 64, 0, 1, 7), (40, 2, 64, 200, 0, 0, 0, 0, 0, 0, 1, 7), (40, 1, 272, 0, 0, 0, 0, 0, 0, 0, 1, 7),
                (40, 1, 64, 0, 0, 0, 0, 0, 0, 0, 1, 9), (40, 1, 64, 0, 0, 0, 0, 0, 0, 0, 3, 7), (40, 1, 64, 0, 3, 64, 64, 0, 0, 0, 1, 7)]:
        assert not ok(*bad), bad
        assert lib.s2d_roi_mlp_packed_elems(*bad) == 0
        assert lib.s2d_roi_mlp_plan_make(*bad, ctypes.byref(_lib.RoiMlpPlan())) != 0 and "unsupported shape" in _lib.last_error()
    plan = _lib.RoiMlpPlan()
    args = (120, 2, 64, 32, 1, 48, 0, 0, 0, 0, 1, 7)
    _lib.check(lib.s2d_roi_mlp_plan_make(*args, ctypes.byref(plan)))
    rows = [(l.cin, l.cout, l.cout_pad, l.relu) for l in plan.layer[:plan.num_layers]]
    assert rows == [(120, 64, 64, 1), (64, 32, 32, 1), (32, 48, 48, 1), (48, 1, 16, 0), (32, 7, 16, 0)]
    assert (plan.n_shared, plan.n_cls, plan.n_reg) == (2, 1, 0)
    w_off, a_off = [0], [0]
    for cin, _, pad, _ in rows:
        w_off.append(w_off[-1] + cin * pad)
        a_off.append(a_off[-1] + 2 * pad)
    assert [l.w_off for l in plan.layer[:5]] == w_off[:-1] and [l.affine_off for l in plan.layer[:5]] == a_off[:-1]
    assert plan.packed_elems == w_off[-1] == lib.s2d_roi_mlp_packed_elems(*args) and plan.affine_elems == a_off[-1]
    # the two-stage configs: 2560 -> 256 -> 256 and two branches 256 -> 256 -> 256 -> {1, 7}
    assert lib.s2d_roi_mlp_packed_elems(2560, 2, 256, 256, 2, 256, 256, 2, 256, 256, 1, 7) == 2560 * 256 + 5 * 256 * 256 + 2 * 256 * 16
