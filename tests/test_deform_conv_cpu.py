"""Deformable convolution v1 and CenterHead(dcn_head=True) without a GPU: state_dict parity with the reference's own head, the
composite path (sparse2dense_amd.dcn.deform_conv_composite) against torch's convolution, against the independent numpy restatement
(tests/dcn_ref.py), under gradcheck and at hand-placed window edges, and the head's forward / loss through the composite."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcn_ref
from sparse2dense_amd import dcn, heads, waymo_configs
from sparse2dense_amd.registry import HEADS, build_from_cfg

REF = "/root/reference"
need_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present")


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def test_dcn_center_head_state_dict_matches_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "dcn_head_keys.npz"))
    cfg = waymo_configs.nusc_centerpoint_dcn()["bbox_head"]
    assert cfg["dcn_head"] is True
    head = build_from_cfg(cfg, HEADS)
    sd = head.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    for (k, v), shape in zip(sd.items(), g["shapes"]):
        assert list(v.shape) == [int(s) for s in shape if s >= 0], k
    for i in range(6):   # the keys the reference's checkpoints carry
        for fa in ("feature_adapt_cls", "feature_adapt_reg"):
            for leaf in ("conv_offset.weight", "conv_offset.bias", "conv_adaption.weight"):
                assert f"tasks.{i}.{fa}.{leaf}" in sd
        assert f"tasks.{i}.cls_head.3.bias" in sd and f"tasks.{i}.task_head.vel.1.running_mean" in sd
    assert head.graph_segment is False
    fa = head.tasks[0].feature_adapt_cls
    assert float(fa.conv_offset.weight.detach().abs().max()) == 0.0
    w = fa.conv_adaption.weight.detach()
    assert float(w.abs().max()) <= 1.0 / (64 * 9) ** 0.5 and float(w.std()) > 0.3 / (64 * 9) ** 0.5
    assert float(head.tasks[1].cls_head[-1].bias.detach()[0]) == pytest.approx(-2.19)
    assert (fa.conv_adaption.deformable_groups, fa.conv_adaption.padding, fa.conv_adaption.kernel_size) == (4, (1, 1), (3, 3))


@need_ref
def test_reference_dcn_config_builds_through_the_shim():
    import sparse2dense_amd.det3d_shim as shim
    shim.install()
    from det3d.models import build_detector
    from det3d.ops.dcn import DeformConv, DeformConvFunction, deform_conv
    from det3d.torchie import Config
    assert DeformConv is dcn.DeformConv and deform_conv is dcn.deform_conv and DeformConvFunction.apply is dcn.deform_conv
    cfg = Config.fromfile(os.path.join(REF, "configs/nusc/voxelnet/nusc_centerpoint_voxelnet_0075voxel_dcn.py"))
    file_head = {k: v for k, v in dict(cfg.model.bbox_head).items()}
    lit = waymo_configs.nusc_centerpoint_dcn()["bbox_head"]
    assert set(file_head) == set(lit)
    for k in lit:
        a, b = file_head[k], lit[k]
        if k == "common_heads":
            assert {h: tuple(v) for h, v in a.items()} == {h: tuple(v) for h, v in b.items()}
        elif k == "tasks":
            assert [dict(t) for t in a] == b
        else:
            assert a == b, k
    det = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert isinstance(det.bbox_head.tasks[5], heads.DCNSepHead)


def test_zero_offsets_equal_the_plain_convolution_exactly():
    x, w = _rand((2, 8, 6, 5), 1), _rand((6, 8, 3, 3), 2)
    off = torch.zeros(2, 2 * 18, 6, 5, dtype=torch.float64)
    y = dcn.deform_conv(x, off, w, 1, 1, 1, 1, 2)
    assert float((y - F.conv2d(x, w, padding=1)).abs().max()) == 0.0
    x = _rand((2, 8, 9, 8), 3)
    off = torch.zeros(2, 18, 3, 2, dtype=torch.float64)
    y = dcn.deform_conv(x, off, w, 2, 0, 2, 1, 1)
    assert float((y - F.conv2d(x, w, stride=2, dilation=2)).abs().max()) == 0.0


def _composite_and_grads(x, off, w, dy, **kw):
    x, off, w = (t.clone().requires_grad_(True) for t in (x, off, w))
    y = dcn.deform_conv_composite(x, off, w, **kw)
    return (y,) + torch.autograd.grad((y * dy).sum(), (x, off, w))


def _check_against_numpy(x, off, w, seed, stride, pad, dil, dg, tol=1e-10):
    y_ref = dcn_ref.forward(x.numpy(), off.numpy(), w.numpy(), stride, pad, dil, 1, dg)
    dy = _rand(y_ref.shape, seed)
    refs = (y_ref,) + dcn_ref.backward(x.numpy(), off.numpy(), w.numpy(), dy.numpy(), stride, pad, dil, 1, dg)
    got = _composite_and_grads(x, off, w, dy, stride=stride, padding=pad, dilation=dil, deformable_groups=dg)
    for name, a, b in zip(("y", "dx", "d_offset", "dw"), got, refs):
        err = float(np.abs(a.detach().numpy() - b).max())
        print(name, err)
        assert np.abs(b).max() > 0 and err <= tol, (name, err)


@pytest.mark.parametrize("case", [dict(shape=(1, 8, 5, 4), cout=6, dg=2, stride=1, pad=1, dil=1),
                                  dict(shape=(2, 16, 6, 7), cout=8, dg=4, stride=2, pad=0, dil=2)])
def test_composite_matches_the_numpy_restatement(case):
    n, c, h, w_ = case["shape"]
    s, p, d, dg = case["stride"], case["pad"], case["dil"], case["dg"]
    ho, wo = (h + 2 * p - (2 * d + 1)) // s + 1, (w_ + 2 * p - (2 * d + 1)) // s + 1
    x, w = _rand(case["shape"], 10), _rand((case["cout"], c, 3, 3), 11)
    off = _rand((n, dg * 18, ho, wo), 12, 1.5)
    _check_against_numpy(x, off, w, 13, s, p, d, dg)


def test_composite_passes_gradcheck():
    x, w = _rand((1, 8, 5, 4), 20).requires_grad_(True), _rand((4, 8, 3, 3), 21).requires_grad_(True)
    off = _rand((1, 2 * 18, 5, 4), 22).requires_grad_(True)   # random real offsets: no position sits on an integer
    assert torch.autograd.gradcheck(lambda a, b, c: dcn.deform_conv_composite(a, b, c, 1, 1, 1, 1, 2), (x, off, w))


def test_window_edges_and_single_corner_placements():
    """offsets chosen so that taps of output pixel (ho, wo) land exactly at -1, H, H-1, 0, -0.5, H-0.5 and far outside"""
    H, W = 5, 4
    x, w = _rand((1, 4, H, W), 30), _rand((3, 4, 3, 3), 31)
    off = torch.zeros(1, 18, H, W, dtype=torch.float64)
    targets = [-1.0, float(H), H - 1.0, 0.0, -0.5, H - 0.5, 1e6, -1e6, 1.25]
    for ho in range(H):
        for wo in range(W):
            for tap in range(9):
                i, j = divmod(tap, 3)
                th = targets[(ho + wo + tap) % len(targets)]
                tw = [-1.0, float(W), W - 1.0, 0.0, -0.5, W - 0.5, 0.5, 2.0, 1e6][(2 * ho + wo + tap) % 9]
                off[0, 2 * tap, ho, wo] = th - (ho - 1 + i)
                off[0, 2 * tap + 1, ho, wo] = tw - (wo - 1 + j)
    # the placements themselves, by value: outside the strict window -> 0, on the last row -> that row, half outside -> half of the edge value
    img = x[0, 0].numpy()
    assert dcn_ref.sample(img, -1.0, 1.0) == 0.0 and dcn_ref.sample(img, float(H), 1.0) == 0.0 and dcn_ref.sample(img, 1e6, 1.0) == 0.0
    assert dcn_ref.sample(img, H - 1.0, 1.0) == img[H - 1, 1] and dcn_ref.sample(img, 0.0, 0.0) == img[0, 0]
    assert dcn_ref.sample(img, -0.5, 2.0) == 0.5 * img[0, 2] and dcn_ref.sample(img, H - 0.5, 2.0) == 0.5 * img[H - 1, 2]
    w1 = torch.zeros(1, 4, 3, 3, dtype=torch.float64)
    w1[0, 0, 0, 0] = 1.0   # the output at (1, 1) is then the sample of channel 0 at tap (0, 0)'s position
    for (th, tw), want in (((-0.5, 2.0), 0.5 * img[0, 2]), ((H - 0.5, 2.0), 0.5 * img[H - 1, 2]), ((-1.0, 1.0), 0.0), ((float(H), 1.0), 0.0),
                           ((H - 1.0, 1.0), img[H - 1, 1]), ((0.0, 0.0), img[0, 0]), ((1e6, 1.0), 0.0)):
        full = dcn.deform_conv_composite(x, _single_tap_offsets(H, W, th, tw), w1, padding=1)
        assert float(full[0, 0, 1, 1]) == pytest.approx(want, abs=1e-15)
    _check_against_numpy(x, off, w, 32, 1, 1, 1, 1)


def _single_tap_offsets(H, W, th, tw):
    """offsets [1, 18, H, W]: tap (0, 0) of output pixel (1, 1) sits at (th, tw); every other tap of every pixel is far outside"""
    off = torch.full((1, 18, H, W), 1e6, dtype=torch.float64)
    off[0, 0, 1, 1] = th - (1 - 1 + 0)
    off[0, 1, 1, 1] = tw - (1 - 1 + 0)
    return off


def test_input_smaller_than_the_kernel_is_padded_and_cropped():
    m = dcn.DeformConv(4, 2, 3, padding=1, deformable_groups=1).double()
    x = _rand((1, 4, 2, 5), 40)
    off = torch.zeros(1, 18, 2, 5, dtype=torch.float64)
    y = m(x, off)
    assert y.shape == (1, 2, 2, 5)
    want = F.conv2d(F.pad(x, (0, 0, 0, 1)), m.weight, padding=1)[:, :, :2]
    assert float((y - want).detach().abs().max()) <= 1e-14


def test_dcn_sep_head_forward_and_loss_on_cpu():
    common = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}
    tasks = [dict(num_class=2, class_names=["a", "b"])]
    head = heads.CenterHead(in_channels=32, tasks=tasks, dataset="nuscenes", weight=0.25, code_weights=[1.0] * 10, common_heads=common,
                            share_conv_channel=64, dcn_head=True)
    assert isinstance(head.tasks[0], heads.DCNSepHead)
    torch.manual_seed(0)
    for t in head.tasks:   # non-zero offsets, so that the offset path carries a gradient
        torch.nn.init.normal_(t.feature_adapt_cls.conv_offset.weight, std=0.05)
        torch.nn.init.normal_(t.feature_adapt_reg.conv_offset.weight, std=0.05)
    n, h, w, m = 2, 12, 10, 6
    x = torch.randn(n, 32, h, w)
    preds = head(x)
    assert len(preds) == 1 and set(preds[0]) == set(common) | {"hm"}
    for k, (c, _) in dict(common, hm=(2, 2)).items():
        assert tuple(preds[0][k].shape) == (n, c, h, w), k
    g = torch.Generator().manual_seed(1)
    example = dict(hm=[torch.rand(n, 2, h, w, generator=g)], anno_box=[torch.randn(n, m, 10, generator=g)],
                   ind=[torch.randint(0, h * w, (n, m), generator=g)], mask=[(torch.rand(n, m, generator=g) > 0.3).to(torch.uint8)],
                   cat=[torch.randint(0, 2, (n, m), generator=g)])
    loss = head.loss(example, preds)["loss"][0]
    assert torch.isfinite(loss)
    loss.backward()
    for fa in (head.tasks[0].feature_adapt_cls, head.tasks[0].feature_adapt_reg):
        gw = fa.conv_offset.weight.grad
        assert gw is not None and torch.isfinite(gw).all() and float(gw.abs().max()) > 0
        assert float(fa.conv_adaption.weight.grad.abs().max()) > 0


def test_relu_sign_flips_of_bf16_storage_alone_exceed_the_gradient_tolerance():
    """Why the GPU tests (tests/test_deform_conv_gpu.py) treat the fused ReLU's mask as an operand of the backward reference.  The float64
    composite with ONLY its sampled columns rounded to bf16 - the one storage rounding every bf16 kernel makes in front of the GEMM - and
    its output stored as bf16 is compared with the exact one at the GPU tests' first shape (2 x 64 x 13 x 11, r = 5): the outputs agree to
    a fraction of the 6e-3 tolerance, a handful of output signs differ, and the exact backward run with that mask instead of its own moves
    dX, d_offset and dW by more than ten times 6e-3 of their maxima (recorded: 9 of 18 304 signs; 6.6e-2, 8.8e-2, 9.4e-2)."""
    import inspect
    src = inspect.getsource(dcn.deform_conv_composite).replace("def deform_conv_composite(", "def rounded_columns(")
    marker = "    col = col.reshape(n, groups, cin_g, k, ho * wo)\n"
    assert marker in src
    scope = dict(vars(dcn))
    exec(src.replace(marker, "    col = col.to(torch.bfloat16).to(dt)\n" + marker), scope)
    g = torch.Generator().manual_seed(0)
    n, c, h, w, r = 2, 64, 13, 11, 5
    x = torch.randn(n, c, h, w, generator=g).bfloat16().double()
    wt = (torch.randn(64, c, 3, 3, generator=g) / 24).bfloat16().double()
    off = torch.randint(-8 * r, 8 * r + 1, (n, 72, h, w), generator=g).double() / 8
    dy = torch.randn(n, 64, h, w, generator=g).bfloat16().double()

    def run(fn, mask=None):
        xx, oo, ww = (t.clone().requires_grad_(True) for t in (x, off, wt))
        y0 = fn(xx, oo, ww, 1, 1, 1, 1, 4)
        y = torch.relu(y0) if mask is None else y0 * mask
        return (y.detach(),) + torch.autograd.grad((y * dy).sum(), (xx, oo, ww))
    exact = run(dcn.deform_conv_composite)
    stored = run(scope["rounded_columns"])[0].bfloat16().double()
    assert float((stored - exact[0]).abs().max() / exact[0].abs().max()) <= 6e-3
    flips = int(((stored > 0) != (exact[0] > 0)).sum())
    assert 0 < flips <= 2e-3 * stored.numel(), flips
    moved = run(dcn.deform_conv_composite, mask=(stored > 0).double())
    for name, a, b in zip(("dX", "d_offset", "dW"), moved[1:], exact[1:]):
        rel = float((a - b).abs().max() / b.abs().max())
        print(name, f"{rel:.2e}", "from", flips, "signs")
        assert rel > 10 * 6e-3, (name, rel)
