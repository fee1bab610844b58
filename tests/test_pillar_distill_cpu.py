"""PointPillars branch of the distillation step (det3d/torchie/trainer/trainer.py:741-773) on the host: the torch restatement of
`heads.pooled_distill_loss`, the dispatch of `train_step.distill_loss` and the `distill=True` pillar frames, against
tests/golden/pillar_distill.npz (the reference's own statements run in float64: tests/golden/make_golden_pillar_distill.py)."""
import numpy as np
import pytest
import torch
from torch import nn

import cpu_backend
from sparse2dense_amd import heads, train_step

MAPS = ("F_S_a", "F_D_a", "F_S_b", "F_D_b")
PILLAR_KEYS = ["T_hm_loss", "kd_hm_loss", "mask_loss", "reconstruction_loss", "sparse2dense_loss"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "pillar_distill.npz"))
    return {k: (torch.from_numpy(g[k]) if g[k].dtype.kind in "fiu" else g[k]) for k in g.files}


def _assert_grad(got, ref):
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert bool((got[ref == 0] == 0).all()), "a position the reference routes no gradient to must hold exactly 0"


def test_fallback_matches_the_reference_statements_in_float64(golden):
    assert list(golden["tied_windows"]) >= [20, 20]
    leaves = [golden[k].clone().requires_grad_(k.startswith("F_S")) for k in MAPS]
    loss = heads.pooled_distill_loss(*leaves)
    assert loss.dtype == torch.float64
    np.testing.assert_allclose(float(loss.detach()), float(golden["log:sparse2dense_loss"]), rtol=1e-12)
    # the golden gradients are those of the whole increment; the heat-map term does not reach the feature maps
    ga, gb = torch.autograd.grad(loss, [leaves[0], leaves[2]])
    _assert_grad(ga, golden["g:F_S_a"])
    _assert_grad(gb, golden["g:F_S_b"])
    for g in (ga, gb):
        assert bool((g[:, :, 6] == 0).all())                       # the odd last row is dropped by the floor-mode pool
        assert int((g != 0).sum()) <= g.shape[0] * g.shape[1] * 3 * 5   # at most one element per 2x2 window
    assert leaves[1].grad is None and leaves[3].grad is None


def test_fallback_empty_class_is_nan(golden):
    zeros = torch.zeros_like(golden["F_D_a"])
    assert torch.isnan(heads.pooled_distill_loss(golden["F_S_a"], zeros, golden["F_S_b"], golden["F_D_b"]))


class PointPillarsScatter(nn.Module):
    """stand-in: only the class name matters (trainer.py:741)"""


class SomeOtherBackbone(nn.Module):
    pass


class _Head:
    code_weights = [1.0] * 8
    weight = 2


class _Teacher(nn.Module):
    def __init__(self, backbone, g):
        super().__init__()
        self.backbone, self.g, self.calls = backbone, g, []

    def forward(self, example, return_loss=True, **kw):
        self.calls.append((return_loss, kw, self.training, torch.is_grad_enabled()))
        hm = self.g["T_hm"]
        box = lambda c, s: torch.randn(2, c, 12, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(s))
        return [dict(hm=hm, reg=box(2, 1), height=box(1, 2), dim=box(3, 3), rot=box(2, 4))], self.g["F_D_a"], self.g["F_D_b"]


class _Student(nn.Module):
    def __init__(self, g):
        super().__init__()
        self.g, self.bbox_head = g, _Head()
        self.leaves = {k: g[k].clone().requires_grad_(True) for k in ("F_S_a", "F_S_b", "S_hm")}

    def forward(self, example, return_loss=True, **kw):
        anno = torch.randn(2, 8, 12, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        return ({"loss": [self.g["base_loss"] * self.leaves["S_hm"].new_ones(())]}, self.leaves["F_S_a"], self.leaves["F_S_b"],
                [dict(hm=self.leaves["S_hm"], anno_box=anno)], self.g["mask_loss"], self.g["offset_loss"])


def _example(g):
    return {k: [g[k]] for k in ("hm", "ind", "mask", "cat")}


def test_distill_loss_takes_the_pillar_branch_for_a_pillar_scatter_teacher(golden):
    teacher, student = _Teacher(PointPillarsScatter(), golden).train(), _Student(golden)
    total, losses = train_step.distill_loss(teacher, student, _example(golden))
    assert teacher.calls == [(False, {}, False, False)]   # T_model(example, return_loss=False), in eval() under no_grad
    assert sorted(k for k in losses if k != "loss") == PILLAR_KEYS == list(golden["log_keys"])
    assert "kd_reg_loss" not in losses
    np.testing.assert_allclose(float(total.detach()), float(golden["base_loss"] + golden["loss_increment"]), rtol=1e-12)
    for k in PILLAR_KEYS:
        v = losses[k][0]
        assert not v.requires_grad
        np.testing.assert_allclose(float(v), float(golden["log:" + k]), rtol=1e-12, err_msg=k)
    grads = torch.autograd.grad(total, [student.leaves[k] for k in ("F_S_a", "F_S_b", "S_hm")])
    for got, k in zip(grads, ("F_S_a", "F_S_b", "S_hm")):
        _assert_grad(got, golden["g:" + k])


def test_distill_loss_keeps_the_centerpoint_branch_for_every_other_teacher(golden):
    teacher, student = _Teacher(SomeOtherBackbone(), golden), _Student(golden)
    total, losses = train_step.distill_loss(teacher, student, _example(golden))
    assert teacher.calls[0][:2] == (False, dict(return_feature=True, return_recon_feature=True))
    assert "kd_reg_loss" in losses and "T_hm_loss" not in losses
    want = heads.sparse2dense_loss(*(golden[k] for k in MAPS))   # 10/20, 5/20 over the unpooled maps
    np.testing.assert_allclose(float(losses["sparse2dense_loss"][0]), float(want), rtol=1e-12)
    assert torch.isfinite(total)


def test_pillar_frames_carry_the_dense_pillars_only_on_request(monkeypatch):
    from sparse2dense_amd.data import SyntheticPillarFrames
    cpu_backend.install(monkeypatch)
    plain = SyntheticPillarFrames(1, n_points=4000, device="cpu").example()
    assert sorted(plain) == sorted(["voxels", "coordinates", "num_points", "num_voxels", "reconstruction_voxels", "reconstruction_coordinates",
                                    "reconstruction_num_points", "reconstruction_num_voxels", "voxel_mean", "reconstruction_voxel_mean", "shape", "hm",
                                    "anno_box", "ind", "mask", "cat"])
    ex = SyntheticPillarFrames(1, n_points=4000, distill=True, device="cpu").example()
    dense = ["dense_voxels", "dense_coordinates", "dense_num_points", "dense_num_voxels"]
    assert set(dense) <= set(ex) and set(plain) <= set(ex)
    assert all(k.startswith("dense_") for k in set(ex) - set(plain))   # (the voxelizer's per-pillar mean rides along, as for the other clouds)
    for prefix in ("dense_", "reconstruction_", ""):
        n = ex[prefix + "voxels"].shape[0]
        assert n > 0 and ex[prefix + "coordinates"].shape == (n, 4) and ex[prefix + "num_points"].shape == (n,)
        assert int(np.sum(np.asarray(ex[prefix + "num_voxels"]))) == n and len(ex[prefix + "num_voxels"]) == 1
        assert ex[prefix + "voxels"].shape[1:] == (20, 5)
    assert ex["dense_voxels"].shape[0] >= ex["voxels"].shape[0]   # the densified cloud holds the sweep
    assert torch.equal(ex["voxels"], plain["voxels"])
