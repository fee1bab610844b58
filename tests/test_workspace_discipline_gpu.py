"""Workspace discipline of every entry that takes a caller-owned scratch buffer (tests/ws_guard.py):

  1. an entry writes every scratch word before it reads it   - the results do not depend on what the buffer held;
  2. an entry touches only the bytes its query asked for     - 4 KiB in front of and at least 4 KiB behind the buffer stay untouched.

Each case calls the public wrapper the family's own test module uses, at shapes of that module's parametrisation: once on the real
allocators (baseline), then with exact-size, guarded workspaces filled with 0xFF (NaN / -1) and with 0x5A (~1.5e16 / a large positive
integer).  The harness must have logged a request from the module the family allocates through (the kernel path ran, not a torch
fallback), both guards of every request must hold, and

  * entries without float atomics (fixed-order folds): every output and gradient of the three runs is bit-identical;
  * entries that accumulate with float atomics (the DCN data gradient, the centre-loss scatters where objects share a cell): the
    atomics' outputs of each of the three runs meet the family's own bound against the family's own float64 reference (imported from
    its test module), everything else is bit-identical.

QUERIES maps each test to the `*_workspace_*` queries whose users it runs (tests/test_ws_guard_cpu.py accounts for all of them)."""
import copy
import os

import numpy as np
import pytest
import torch

import ws_guard

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
QUERIES = {}


def queries(*names):
    def deco(fn):
        QUERIES[fn.__name__] = names
        return fn
    return deco


def _snap(out):
    """detached copies of a run's outputs: {name: tensor}"""
    flat = {}
    for k, v in out.items():
        if v is None:
            continue
        if torch.is_tensor(v):
            flat[k] = v.detach().clone()
        else:
            for i, t in enumerate(v):
                if t is not None:
                    flat[f"{k}[{i}]"] = t.detach().clone()
    return flat


def _same(t, ref):
    """bit-equal; a NaN of the baseline (the mean over no voxels of an empty frame) must be a NaN again"""
    if not t.is_floating_point() or not bool(ref.isnan().any()):
        return torch.equal(t, ref)
    return torch.equal(t.isnan(), ref.isnan()) and torch.equal(torch.where(t.isnan(), 0, t), torch.where(ref.isnan(), 0, ref))


def discipline(monkeypatch, run, modules, bounded=(), check=None):
    """run() -> {name: tensor | list of tensors}.  `bounded`: names (prefixes) of outputs that float atomics accumulate - held by
    `check(outputs)` (the family's bound against its float64 reference) on every run instead of bit-equality."""
    base = _snap(run())
    torch.cuda.synchronize()
    runs = {"baseline": base}
    for poison in ws_guard.POISONS:
        with ws_guard.guard(monkeypatch, poison) as log:   # leaving the block synchronises and checks both guards of every request
            got = _snap(run())
        runs[f"poison {poison:#x}"] = got
        assert log.requests, "no workspace was requested: the kernel path was not taken"
        missing = set(modules) - log.modules()
        assert not missing, f"no workspace request from {sorted(missing)} (requests: {log.requests})"
        assert all(n > 0 for m, n in log.requests if m in modules), log.requests
    is_bounded = lambda name: any(name == b or name.startswith(b + "[") for b in bounded)
    for tag, got in runs.items():
        assert set(got) == set(base), tag
        for name, t in got.items():
            ref = base[name]
            assert t.shape == ref.shape and t.dtype == ref.dtype, (tag, name)
            if t.is_floating_point():
                assert bool((torch.isfinite(t) | ~torch.isfinite(ref)).all()), f"{tag}: {name} is not finite where the baseline is"
            if not is_bounded(name):
                assert _same(t, ref), f"{tag}: {name} differs from the baseline (max |diff| {float((t.double() - ref.double()).abs().max()):.3e})"
        if check is not None:
            check(got)
    assert bounded == () or check is not None


def _nhwc16(t):
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grads(mods):
    return [p.grad for m in mods if m is not None for p in m.parameters()]


# ---- dense 2-D weight gradients ---------------------------------------------------------------------------------------------------
@queries("s2d_conv2d3x3_wgrad_workspace_bytes")
@pytest.mark.parametrize("n,cin,cout,h,w,pad", [(1, 128, 192, 17, 19, 0), (2, 64, 64, 20, 24, 1)])
def test_conv3x3_wgrad(n, cin, cout, h, w, pad, monkeypatch):
    from sparse2dense_amd import dense2d as D
    g = _gen(3)
    x = _nhwc16(torch.randn(n, cin, h, w, generator=g).to(DEV))
    dy = _nhwc16(torch.randn(n, cout, h + 2 * pad - 2, w + 2 * pad - 2, generator=g).to(DEV))
    discipline(monkeypatch, lambda: {"dw": D.conv3x3_wgrad(x, dy, pad)}, ["dense2d"])


def _module_case(make, x, dy, autocast=True):
    """forward + backward of a dense2d module under bf16 autocast on fresh copies of the same parameters"""
    proto = make()

    def run():
        m = copy.deepcopy(proto).to(DEV)
        xa = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = m(xa)
        y.backward(dy.to(y.dtype))
        return {"y": y, "dx": xa.grad, "dparams": _grads([m]), "buffers": list(m.buffers())}
    return run


@queries("s2d_conv2d1x1_wgrad_workspace_bytes")
@pytest.mark.parametrize("n,cin,cout,h,w", [(1, 64, 64, 5, 7), (2, 256, 640, 33, 20)])
def test_conv1x1_wgrad(n, cin, cout, h, w, monkeypatch):
    from sparse2dense_amd import dense2d as D
    torch.manual_seed(n + cin + cout)
    x = torch.randn(n, cin, h, w, device=DEV).to(torch.bfloat16).float().contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, cout, h, w, device=DEV)
    discipline(monkeypatch, _module_case(lambda: D.Conv1x1(cin, cout, 1, 1, 0, bias=True), x, dy), ["dense2d"])


@queries("s2d_conv2d_s2_wgrad_workspace_bytes")
@pytest.mark.parametrize("kind,n,h,w,cin,cout", [("k4", 3, 5, 3, 128, 128), ("k3", 2, 9, 6, 64, 192)])
def test_stride2_wgrad(kind, n, h, w, cin, cout, monkeypatch):
    """k4: the weight gradient of ConvTranspose2d(4,2,1); k3: of the stride-2 3x3 conv (both csrc/conv2d_wgrad.hip, STRIDE = 2)"""
    from sparse2dense_amd import dense2d as D
    g = _gen(n * 77 + h)
    if kind == "k4":
        a = _nhwc16(torch.randn(n, cin, h, w, generator=g).to(DEV))
        b = _nhwc16(torch.randn(n, cout, 2 * h, 2 * w, generator=g).to(DEV))
        run = lambda: {"dw": D.conv_s2_wgrad(a, b, 4)}
    else:
        x = _nhwc16(torch.randn(n, cin, 2 * h, 2 * w, generator=g).to(DEV))
        dy = _nhwc16(torch.randn(n, cout, h, w, generator=g).to(DEV))
        run = lambda: {"dw": D.conv_s2_wgrad(dy, x, 3)}
    discipline(monkeypatch, run, ["dense2d"])


@queries("s2d_smallconv3x3_wgrad_workspace_bytes")
@pytest.mark.parametrize("n,cin,cout,h,w", [(1, 64, 2, 7, 5), (2, 128, 4, 19, 30)])
def test_small_cout_conv3x3(n, cin, cout, h, w, monkeypatch):
    from sparse2dense_amd import dense2d as D
    torch.manual_seed(n + cin + cout + h)
    x = torch.randn(n, cin, h, w, device=DEV).to(torch.bfloat16).float().contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, cout, h, w, device=DEV)
    discipline(monkeypatch, _module_case(lambda: D.SmallConv3x3(cin, cout, 3, 1, 1, bias=True), x, dy), ["dense2d"])


@queries("s2d_dwconv7_wgrad_workspace_bytes")
@pytest.mark.parametrize("n,c,h,w", [(1, 64, 9, 5), (2, 8, 20, 33)])
def test_depthwise7(n, c, h, w, monkeypatch):
    from sparse2dense_amd import dense2d as D
    torch.manual_seed(4)
    x = torch.randn(n, c, h, w, device=DEV).to(torch.bfloat16).float()
    dy = torch.randn(n, c, h, w, device=DEV)
    discipline(monkeypatch, _module_case(lambda: D.DepthwiseConv7(c, c, 7, padding=3, groups=c, bias=True), x, dy), ["dense2d"])


# ---- batch norms and layer norm ---------------------------------------------------------------------------------------------------
@queries("s2d_bnrow_workspace_bytes")
@pytest.mark.parametrize("case", [("2d", 2, 8, 5, 7, True), ("2d", 1, 256, 33, 9, 2), ("2d", 1, 8, 1, 1, False),
                                  ("rows", 33, 32, True), ("rows", 777, 128, True), ("rows", 1, 16, False)], ids=str)
def test_batchnorm2d_rows(case, monkeypatch):
    """FastBatchNorm2d in training (statistics, apply, backward reduction) and the bf16 feature rows with residual + ReLU; one row is
    the degenerate case"""
    from sparse2dense_amd import dense2d as D
    torch.manual_seed(2)
    if case[0] == "2d":
        _, n, c, h, w, relu = case
        x = _nhwc16(torch.randn(n, c, h, w, device=DEV) * 2 + 0.3)
        dy = _nhwc16(torch.randn(n, c, h, w, device=DEV))

        def make():
            m = D.FastBatchNorm2d(c, eps=1e-3, momentum=0.01, fused_relu=relu)
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5)
            return m
        run = _module_case(make, x, dy, autocast=False)
    else:
        from sparse2dense_amd.spconv import FeatureBatchNorm1d
        _, n, c, with_res = case
        proto = FeatureBatchNorm1d(c, eps=1e-3, momentum=0.01)
        with torch.no_grad():
            proto.weight.uniform_(0.5, 1.5); proto.bias.uniform_(-0.5, 0.5)
        x = (torch.randn(n, c, device=DEV) * 2 + 0.3).to(torch.bfloat16)
        res = torch.randn(n, c, device=DEV).to(torch.bfloat16) if with_res else None
        dy = torch.randn(n, c, device=DEV).to(torch.bfloat16)

        def run():
            m = copy.deepcopy(proto).to(DEV)
            xa = x.clone().requires_grad_(True)
            ra = res.clone().requires_grad_(True) if with_res else None
            y = m(xa, residual=ra, relu=True)
            y.backward(dy)
            return {"y": y, "dx": xa.grad, "dres": None if ra is None else ra.grad, "dparams": _grads([m]), "buffers": list(m.buffers())}
    discipline(monkeypatch, run, ["dense2d"])


@queries("s2d_bn_partials_sum_workspace_bytes", "s2d_bnrow_workspace_bytes")
@pytest.mark.parametrize("nblocks,c", [(5000, 16), (9000, 128), (777, 16)])
def test_partial_fold(nblocks, c, monkeypatch):
    """the batch norm fed with per-tile (sum, sum of squares) rows from a producer's epilogue: the fold of the list (two stages above
    1536 rows - a workspace of its own when it does not fit the row kernels' one; one stage for the short list) instead of a statistics
    pass.  One row per tile, so the list is exactly consistent with x."""
    from sparse2dense_amd import _lib
    from sparse2dense_amd.spconv import FeatureBatchNorm1d
    assert (_lib.load().s2d_bn_partials_sum_workspace_bytes(nblocks, c) > 0) == (nblocks > 1536)
    torch.manual_seed(nblocks % 97 + c)
    proto = FeatureBatchNorm1d(c, eps=1e-3, momentum=0.01)
    x = (torch.randn(nblocks, c, device=DEV) * 2 + 0.3).to(torch.bfloat16)
    partial = torch.stack([x.float(), x.float() ** 2], 1).contiguous()   # [tiles, 2, c]
    dy = torch.randn(nblocks, c, device=DEV).to(torch.bfloat16)

    def run():
        m = copy.deepcopy(proto).to(DEV)
        xa = x.clone().requires_grad_(True)
        xa._s2d_bn_partial = partial
        y = m(xa, relu=True)
        y.backward(dy)
        return {"y": y, "dx": xa.grad, "dparams": _grads([m]), "buffers": list(m.buffers())}
    first = run()   # the list was used, and used right: the running mean moved by momentum * the mean of the rows
    want = 0.01 * x.double().mean(0)
    assert (first["buffers"][0].double() - want).abs().max() <= 1e-5 * want.abs().max() + 1e-7
    discipline(monkeypatch, run, ["dense2d"])


@queries("s2d_bn_partials_sum_workspace_bytes", "s2d_bnrow_workspace_bytes", "s2d_conv2d3x3_wgrad_workspace_bytes",
         "s2d_conv2d1x1_wgrad_workspace_bytes")
@pytest.mark.parametrize("kind,c0,c1,c2,hw", [("3x3", 64, 128, 128, (37, 29)), ("1x1", 128, 256, 128, (33, 20))])
def test_conv_bn_chain_folds(kind, c0, c1, c2, hw, monkeypatch):
    """conv -> BN -> ReLU -> conv -> BN -> ReLU: the forward statistics come from the convs' epilogue rows and the first batch norm's
    backward sums from the second conv's data-gradient epilogue - both lists are folded through a workspace"""
    from sparse2dense_amd import dense2d as D
    conv = (lambda ci, co: D.Conv1x1(ci, co, 1, bias=False)) if kind == "1x1" else (lambda ci, co: D.Conv3x3(ci, co, 3, padding=1, bias=False))
    torch.manual_seed(11)
    net = torch.nn.Sequential(*D.fuse_bn_relu([conv(c0, c1), D.FastBatchNorm2d(c1, eps=1e-3, momentum=0.01), torch.nn.ReLU(),
                                               conv(c1, c2), D.FastBatchNorm2d(c2, eps=1e-3, momentum=0.01), torch.nn.ReLU()])).train()
    assert net[0].emit_bn_stats
    with torch.no_grad():
        for m in net:
            if isinstance(m, D.FastBatchNorm2d):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5)
    x = _nhwc16(torch.randn(3, c0, *hw, device=DEV))
    monkeypatch.setattr(D, "BN_BWD_FOLD", 1)   # (opt-in in the product: S2D_BN_BWD_FOLD)

    def run():
        m = copy.deepcopy(net).to(DEV)
        for k in D.STATS:
            D.STATS[k] = 0
        xi = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(xi)
        (y.float() * torch.linspace(-1, 1, y.shape[-1], device=DEV)).sum().backward()
        assert D.STATS["bn_bwd_folded"] == 1 and D.STATS["bn_bwd_reduced"] == 1, D.STATS
        return {"y": y, "dx": xi.grad, "dparams": _grads([m]), "buffers": list(m.buffers())}
    discipline(monkeypatch, run, ["dense2d"])


@queries("s2d_bn1d_workspace_bytes")
@pytest.mark.parametrize("n,c", [(1, 16), (777, 16), (3000, 128)])
def test_bn1d(n, c, monkeypatch):
    from sparse2dense_amd import hip_ops as H
    torch.manual_seed(n + c)
    x = (torch.randn(n, c) * 2 + 0.5).to(DEV)
    dy, y = torch.randn(n, c).to(DEV), torch.randn(n, c).to(DEV)
    gamma, beta = (torch.rand(c) + 0.5).to(DEV), (torch.randn(c) * 0.1).to(DEV)

    def run():
        rm, rv, nbt = torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
        fin = H.bn1d_stats_finalize(x, gamma, beta, 1e-3, 0.01, rm, rv, nbt)
        g, sums = H.bn1d_bwd_reduce(dy, y, x, True)
        g2, out = H.bn1d_bwd_reduce_finalize(dy, y, x, True, gamma, fin[0].contiguous(), fin[1].contiguous())
        return {"stats": H.bn1d_stats(x), "fin": fin, "running": [rm, rv, nbt], "g": g, "sums": sums, "g2": g2, "bwd": out}
    discipline(monkeypatch, run, ["hip_ops"])


@queries("s2d_lnwide_workspace_bytes")
@pytest.mark.parametrize("n,c,h,w,nhwc", [(3, 8, 96, 100, True), (2, 64, 47, 47, False)])
def test_wide_layernorm(n, c, h, w, nhwc, monkeypatch):
    from sparse2dense_amd import dense2d as D
    torch.manual_seed(7)
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    x = (torch.randn(n, c, h, w, device=DEV) * 2 + 0.5).to(torch.bfloat16).contiguous(memory_format=fmt)
    dy = torch.randn(n, c, h, w, device=DEV).to(torch.bfloat16).contiguous(memory_format=fmt)
    proto = D.WideLayerNorm([c, h, w], eps=1e-6)
    with torch.no_grad():
        proto.weight.uniform_(0.5, 1.5); proto.bias.uniform_(-1, 1)

    def run():
        m = copy.deepcopy(proto).to(DEV)
        xa = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y = m(xa)
        assert y.dtype == torch.bfloat16   # the bf16 kernels, not the stock layer
        y.backward(dy)
        return {"y": y, "dx": xa.grad, "dparams": _grads([m])}
    discipline(monkeypatch, run, ["dense2d"])


@queries("s2d_bncm_workspace_bytes")
@pytest.mark.parametrize("c,shape", [(3, (2, 20, 24, 28)), (32, (2, 5, 12, 16)), (8, (1, 1, 1, 4))])
def test_bn3d_channel_major(c, shape, monkeypatch):
    from sparse2dense_amd.dense3d import FastBatchNorm3d
    torch.manual_seed(c)
    n, d, h, w = shape
    x = (torch.randn(n, c, d, h, w) * 2 + 0.3).to(DEV)
    dy = torch.randn(n, c, d, h, w, generator=_gen(1)).to(DEV)
    proto = FastBatchNorm3d(c, eps=1e-5, momentum=0.1, fused_relu=True)
    with torch.no_grad():
        proto.weight.uniform_(0.5, 1.5); proto.bias.normal_(0, 0.2)

    def run():
        m = copy.deepcopy(proto).to(DEV).train()
        xa = x.clone().requires_grad_(True)
        y = m(xa)
        y.backward(dy)
        return {"y": y, "dx": xa.grad, "dparams": _grads([m]), "buffers": list(m.buffers())}
    discipline(monkeypatch, run, ["dense3d"])


# ---- dense 3-D weight gradients ---------------------------------------------------------------------------------------------------
@queries("s2d_pointwise_conv_wgrad_workspace_bytes")
@pytest.mark.parametrize("cin,cout,shape,bf16", [(32, 16, (1, 3, 5, 4), False), (128, 32, (2, 5, 12, 16), False), (32, 16, (1, 3, 5, 4), True),
                                                 (128, 32, (2, 5, 12, 16), True)])
def test_pointwise_conv3d_wgrad(cin, cout, shape, bf16, monkeypatch):
    from sparse2dense_amd.dense3d import PointwiseConv3d
    torch.manual_seed(cin + 3 * cout)
    n, d, h, w = shape
    x, dy = torch.randn(n, cin, d, h, w).to(DEV), torch.randn(n, cout, d, h, w).to(DEV)
    proto = PointwiseConv3d(cin, cout, 1, 1, 0)

    def run():
        m = copy.deepcopy(proto).to(DEV)
        m.bf16_compute = bf16
        xa = x.clone().requires_grad_(True)
        y = m(xa)
        y.backward(dy)
        return {"y": y, "dx": xa.grad, "dparams": _grads([m])}
    discipline(monkeypatch, run, ["dense3d"])


def _level_modules(cin, cout, gen, pre):
    from torch import nn
    from sparse2dense_amd.dense3d import ConvTranspose3dK4S2, FastBatchNorm3d
    pre_bn = None
    if pre:
        pre_bn = FastBatchNorm3d(cin, fused_relu=True)
        with torch.no_grad():
            pre_bn.weight.copy_(torch.rand(cin, generator=gen) + 0.5)
            pre_bn.bias.copy_(torch.randn(cin, generator=gen) * 0.3)
    return [pre_bn, ConvTranspose3dK4S2(cin, cout, 4, 2, 1), FastBatchNorm3d(cout, fused_relu=True), nn.Conv3d(cout, 1, 1), nn.Conv3d(cout, 3, 1)]


@queries("s2d_convt3d_mfma_wgrad_workspace_bytes", "s2d_pcr_level_workspace_bytes", "s2d_bncm_workspace_bytes")
@pytest.mark.parametrize("site,cin,cout,shape", [("f32", 16, 3, (1, 2, 3, 24)), ("f32", 32, 32, (2, 3, 6, 70)),
                                                 ("d16", 16, 3, (1, 2, 3, 24)), ("d16", 32, 32, (2, 3, 6, 12)),
                                                 ("d16_norm", 16, 3, (1, 2, 3, 24)), ("d16_norm", 16, 3, (2, 3, 5, 16)),
                                                 ("d16_norm_x16", 16, 3, (1, 2, 3, 24)), ("d16_norm_x16", 16, 3, (2, 4, 6, 16))])
def test_convt3d_mfma_wgrad(site, cin, cout, shape, monkeypatch):
    """the four weight-gradient launches of the matrix-core ConvTranspose3d(4,2,1) backward: fp32 gradient in (the plain layer); and,
    through heads.upsample_level, the bf16 gradient, the bf16 gradient with the batch norm in front folded in, and that with a bf16 input.
    (The bf16-gradient kernels need a row length that is a multiple of 4, the folded ones of 8: (2, 3, 6, 70) serves the fp32 site only, the
    others take the second shapes of tests/test_losses_gpu.py's up-sampler tests.)"""
    from sparse2dense_amd import dense3d, heads
    import test_losses_gpu as TL
    n, d, h, w = shape
    gen = _gen(5 + cin + w)
    entries = []
    real_check = dense3d.check
    monkeypatch.setattr(dense3d, "check", lambda rc, name: (entries.append(name), real_check(rc, name))[1])
    want = {"f32": "s2d_convt3d_mfma_wgrad", "d16": "s2d_convt3d_mfma_wgrad_d16", "d16_norm": "s2d_convt3d_mfma_wgrad_d16_norm",
            "d16_norm_x16": "s2d_convt3d_mfma_wgrad_d16_norm_x16"}[site]
    if site == "f32":
        x0 = torch.randn(n, cin, d, h, w, generator=gen)
        dy = torch.randn(n, cout, 2 * d, 2 * h, 2 * w, generator=gen).to(DEV)
        proto = dense3d.ConvTranspose3dK4S2(cin, cout, 4, 2, 1)

        def run():
            m = copy.deepcopy(proto).to(DEV)
            m.bf16_compute = True
            xa = x0.to(DEV).requires_grad_(True)
            y = m(xa)
            y.backward(dy)
            return {"y": y, "dx": xa.grad, "dparams": _grads([m])}
    else:
        m_sites = 90 if n == 1 else 900
        coors, feats, _, _ = TL._case(n, 2 * d, 2 * h, 2 * w, m_sites, seed=cin + cout + m_sites)
        coors, feats = coors.to(DEV), feats.to(DEV)
        x0 = torch.randn(n, cin, d, h, w, generator=gen) * 1.3 + 0.4
        mods0 = _level_modules(cin, cout, gen, pre=site != "d16")
        x16 = site == "d16_norm_x16"
        if x16:
            x0 = x0.to(torch.bfloat16)
            xf = x0.double()
            stats = torch.cat([xf.sum(dim=(0, 2, 3, 4)), (xf * xf).sum(dim=(0, 2, 3, 4))]).float().to(DEV)

        def run():
            mods = [None if mm is None else copy.deepcopy(mm).to(DEV) for mm in mods0]
            mods[1].bf16_compute = True
            for mm in (mods[0], mods[2]):
                if mm is not None:
                    mm.train()
            assert heads.upsample_level_supported(mods[1], (d, h, w), None)
            if mods[0] is not None:
                assert heads.upsample_level_pre_bn_supported(mods[1], (d, h, w), mods[0])
            xa = x0.to(DEV).requires_grad_(True)
            if x16:
                assert heads.upsample_level_x16_supported(mods[1], (d, h, w), mods[0])
                xa._s2d_bn_stats = stats
            ml, ol, _ = heads.upsample_level(mods[1], xa, mods[2], mods[3], mods[4], coors, feats, pre_bn=mods[0])
            (1.7 * ml + 0.6 * ol).backward()
            return {"losses": [ml, ol], "dx": xa.grad, "dparams": _grads(mods), "buffers": [b for mm in mods if mm is not None for b in mm.buffers()]}
    discipline(monkeypatch, run, ["dense3d"] if site == "f32" else ["dense3d", "dense2d"])
    assert {e for e in entries if "mfma_wgrad" in e} == {want}, entries


@queries("s2d_convt3d_k4s2p1_wgrad_workspace_bytes")
@pytest.mark.parametrize("cin,cout,shape", [(1, 1, (1, 1, 1, 2)), (4, 5, (2, 2, 5, 6))])
def test_convt3d_f32_wgrad(cin, cout, shape, monkeypatch):
    from sparse2dense_amd.dense3d import ConvTranspose3dK4S2
    torch.manual_seed(cin * 3 + cout)
    n, d, h, w = shape
    x = torch.randn(n, cin, d, h, w).to(DEV)
    dy = torch.randn(n, cout, 2 * d, 2 * h, 2 * w, generator=_gen(3)).to(DEV)
    proto = ConvTranspose3dK4S2(cin, cout, 4, 2, 1)

    def run():
        m = copy.deepcopy(proto).to(DEV)
        xa = x.clone().requires_grad_(True)
        y = m(xa)
        y.backward(dy)
        return {"y": y, "dx": xa.grad, "dparams": _grads([m])}
    discipline(monkeypatch, run, ["dense3d"])


# ---- sparse weight gradients ------------------------------------------------------------------------------------------------------
@queries("s2d_spconv_wgrad_workspace_bytes")
@pytest.mark.parametrize("cin,cout", [(16, 16), (128, 128)])
@pytest.mark.parametrize("n_out,p_empty", [(63, 0.5), (4097, 0.97), (70, 1.0)])
def test_sparse_conv_wgrad(cin, cout, n_out, p_empty, monkeypatch):
    """the fp32 and the bf16-storage weight gradients over the same map; an all-empty map is the degenerate case"""
    from sparse2dense_amd import hip_ops as H
    import test_s16_gpu as TS
    torch.manual_seed(11)
    n_in, kvol = 1500, 27
    feat = torch.randn(n_in, cin, device=DEV)
    dout = torch.randn(n_out, cout, device=DEV)
    nbr = TS._random_map(kvol, n_in, n_out, p_empty=p_empty, seed=5)
    f16, d16 = feat.to(torch.bfloat16), dout.to(torch.bfloat16)
    discipline(monkeypatch, lambda: {"dw_f32": H.spconv_wgrad(feat, dout, nbr, kvol), "dw_s16": H.spconv_s16_wgrad(f16, d16, nbr, kvol)},
               ["hip_ops"])


@queries("s2d_rows_wgrad_workspace_bytes")
@pytest.mark.parametrize("rows,ci,co", [(7, 64, 64), (5000, 33, 17)])
def test_pillar_rows_wgrad(rows, ci, co, monkeypatch):
    from sparse2dense_amd import pillars as P
    g = _gen(rows)
    x0 = torch.randn(rows, ci, generator=g).to(DEV)
    w0 = (torch.randn(co, ci, generator=g) * 0.2).to(DEV)
    dy = torch.randn(rows, co, generator=g).to(DEV)

    def run():
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        y = P._RowLinearFn.apply(x, w)
        y.backward(dy)
        return {"y": y, "dx": x.grad, "dw": w.grad}
    discipline(monkeypatch, run, ["dense2d"])


# ---- fused losses -----------------------------------------------------------------------------------------------------------------
@queries("s2d_focal_workspace_bytes")
@pytest.mark.parametrize("b,c,h,w,m,n_pos", [(2, 1, 9, 7, 16, 5), (1, 3, 20, 12, 8, 0), (3, 2, 33, 40, 64, 64)])
def test_focal(b, c, h, w, m, n_pos, monkeypatch):
    """value bit-identical; the gradient's positive part is scattered with float atomics and two objects share a cell: it is held to the
    bound of tests/test_losses_gpu.py against its float64 reference on every run"""
    import test_losses_gpu as TL
    from sparse2dense_amd.heads import fast_focal_loss
    g = _gen(b * 100 + c * 10 + m)
    out = torch.rand(b, c, h, w, generator=g).clamp(1e-4, 1 - 1e-4)
    target = torch.rand(b, c, h, w, generator=g) ** 3
    ind = torch.randint(0, h * w, (b, m), generator=g)
    cat = torch.randint(0, c, (b, m), generator=g)
    ind[:, 1], cat[:, 1] = ind[:, 0], cat[:, 0]
    mask = torch.zeros(b, m, dtype=torch.uint8)
    mask.view(-1)[torch.randperm(b * m, generator=g)[:n_pos]] = 1
    if n_pos >= 2:
        mask[0, 0] = mask[0, 1] = 1
    od = out.double().requires_grad_(True)
    ref = TL._focal_ref(od, target.double(), ind, mask, cat)
    ref.backward()
    dev = [t.to(DEV) for t in (target, ind, mask, cat)]

    def run():
        oc = out.to(DEV).requires_grad_(True)
        got = fast_focal_loss(oc, *dev)
        (got * 1.7).backward()
        return {"loss": got, "dout": oc.grad}

    def check(o):
        assert abs(o["loss"].item() - ref.item()) <= 2e-5 * abs(ref.item())
        gref = od.grad * 1.7
        assert (o["dout"].cpu().double() - gref).abs().max() <= 1e-4 * gref.abs().max()
    discipline(monkeypatch, run, ["dense2d"], bounded=("dout",), check=check)


@queries("s2d_center_tasks_loss_workspace_bytes")
@pytest.mark.parametrize("positives", ["some", "none"])
@pytest.mark.parametrize("table,vel,b,h,w,m", [([3, 1], False, 2, 9, 7, 16), ([1, 2, 2, 1, 2, 2], True, 2, 9, 7, 16),
                                                ([3, 1], False, 3, 33, 40, 64)])
def test_center_tasks_loss(table, vel, b, h, w, m, positives, monkeypatch):
    """forward results bit-identical; the gradients are scattered with float atomics and objects 0 and 1 of every frame share a cell:
    held to the bounds of tests/test_center_tasks_loss_gpu.py against its float64 loop on every run"""
    import test_center_tasks_loss_gpu as TC
    preds, ex, names = TC._case(table, vel, b, h, w, m, seed=b * 1000 + h * 10 + len(table), positives=positives)
    nch = 10 if vel else 8
    cw = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0][:nch] if vel else [1.0, 0.5, 1.0, 2.0, 1.0, 1.0, 0.3, 1.0]
    factors = [1.0 + 0.37 * t for t in range(len(table))]
    leaves64 = [{k: v.double().requires_grad_(True) for k, v in p.items()} for p in preds]
    ref = TC._ref_loop(ex, leaves64, cw, 0.25)
    sum(f * r["loss"] for f, r in zip(factors, ref)).backward()

    def run():
        loss, loc, res, probs, leaves = TC._run_node(preds, ex, names, cw, 0.25, factors)
        out = {"loss": loss, "loc": loc, "res": res, "probs": probs}
        for k in ["hm"] + names:
            out["d_" + k] = [lv[k].grad for lv in leaves]
        return out

    def check(o):
        for t, r in enumerate(ref):
            assert abs(float(o["loss"][t]) - float(r["loss"].detach())) <= 2e-5 * abs(float(r["loss"].detach())) + 1e-12, t
            for k in ["hm"] + names:
                got, want = o[f"d_{k}[{t}]"].cpu().double(), leaves64[t][k].grad
                assert (got - want).abs().max() <= (1e-4 if k == "hm" else 1e-5) * want.abs().max() + 1e-15, (t, k)
    discipline(monkeypatch, run, ["dense2d"], bounded=tuple("d_" + k for k in ["hm"] + names), check=check)


@queries("s2d_masked_mse_workspace_bytes")
@pytest.mark.parametrize("sdt,tdt,cl", [(torch.bfloat16, torch.bfloat16, True), (torch.float32, torch.float32, False)])
@pytest.mark.parametrize("shape", [(2, 8, 5, 12), (4, 64, 47, 48)])
def test_masked_mse(shape, sdt, tdt, cl, monkeypatch):
    from sparse2dense_amd import heads
    g = _gen(3)
    fmt = torch.channels_last if cl else torch.contiguous_format
    s0 = torch.randn(shape, generator=g).to(sdt).contiguous(memory_format=fmt).to(DEV)
    t0 = torch.randn(shape, generator=g).relu().to(tdt).contiguous(memory_format=fmt).to(DEV)

    def run():
        sh = s0.clone(memory_format=torch.preserve_format).requires_grad_(True)
        out = heads.masked_mse_pair(sh, t0, 10.0, 20.0)
        assert "_MaskedMseFn" in type(out.grad_fn).__name__
        (out * 1.0).backward()
        return {"loss": out, "ds": sh.grad}
    discipline(monkeypatch, run, ["dense2d"])


@queries("s2d_pooled_distill_workspace_bytes")
@pytest.mark.parametrize("shape", [(1, 8, 2, 2), (2, 64, 9, 13)])
@pytest.mark.parametrize("combo", [("bf16", "cl", "f32", "nchw"), ("f32", "nchw", "f32", "nchw")], ids="-".join)
def test_pooled_distill(combo, shape, monkeypatch):
    import test_pillar_distill_gpu as TP
    monkeypatch.delenv("S2D_PILLAR_DISTILL_FUSED", raising=False)
    case = TP._case(shape, combo[0], combo[2])

    def run():
        loss, ga, gb, _, _ = TP._run(case, combo)
        return {"loss": loss, "ga": ga, "gb": gb}
    discipline(monkeypatch, run, ["dense2d"])


@queries("s2d_pcr_loss_workspace_bytes")
@pytest.mark.parametrize("b,d,h,w,m", [(1, 5, 17, 9, 40), (2, 6, 20, 24, 300), (1, 5, 17, 9, 0)])
def test_pcr_loss(b, d, h, w, m, monkeypatch):
    import test_losses_gpu as TL
    from sparse2dense_amd import heads
    coors, feats, gen_off, gen_mask = TL._case(b, d, h, w, m, seed=b * 7 + m)
    coors, feats = coors.to(DEV), feats.to(DEV)

    def run():
        go, gm = gen_off.to(DEV).requires_grad_(True), gen_mask.to(DEV).requires_grad_(True)
        ml, ol = heads.mask_offset_loss_sparse(go, gm, coors, feats)
        (1.7 * ml + 0.6 * ol).backward()
        return {"losses": [ml, ol], "d_off": go.grad, "d_mask": gm.grad}
    discipline(monkeypatch, run, ["dense2d"])


def _pcr_level_case(b, c, co, d, h, w, m, norm):
    import test_losses_gpu as TL
    from torch import nn
    from sparse2dense_amd import heads
    from sparse2dense_amd.dense3d import FastBatchNorm3d
    coors, feats, _, _ = TL._case(b, d, h, w, m, seed=b * 11 + m + c)
    coors, feats = coors.to(DEV), feats.to(DEV)
    gen = _gen(5 + c + m)
    g0 = torch.randn(b, c, d, h, w, generator=gen)
    g0 = g0 * 1.5 + 0.2 if norm else g0.relu()
    mods0 = [FastBatchNorm3d(c, fused_relu=True) if norm else None, nn.Conv3d(c, 1, 1), nn.Conv3d(c, 3, 1), nn.Conv3d(c, co, 1) if co else None]
    r = (torch.randn(b, co, d, h, w, generator=gen) / (b * d * h * w)).to(DEV) if co else None

    def run():
        mods = [None if mm is None else copy.deepcopy(mm).to(DEV) for mm in mods0]
        g = g0.to(DEV).requires_grad_(True)
        if norm:
            mods[0].train()
            ml, ol, z = heads.pcr_level_norm(g, mods[0], mods[1], mods[2], coors, feats, next_conv=mods[3])
        else:
            assert heads.pcr_level_supported(g, mods[3])
            ml, ol, z = heads.pcr_level(g, mods[1], mods[2], coors, feats, next_conv=mods[3])
        total = 1.7 * ml + 0.6 * ol
        if co:
            total = total + (z * r).sum()
        total.backward()
        return {"losses": [ml, ol], "z": z, "dg": g.grad, "dparams": _grads(mods), "buffers": [] if not norm else list(mods[0].buffers())}
    return run


PCR_LEVEL_CASES = [(1, 32, 0, 4, 10, 12, 50), (2, 3, 0, 6, 20, 24, 300), (2, 32, 16, 6, 20, 24, 300), (1, 3, 0, 4, 10, 12, 0)]


@queries("s2d_pcr_heads_workspace_bytes", "s2d_pointwise_conv_wgrad_workspace_bytes")
@pytest.mark.parametrize("b,c,co,d,h,w,m", PCR_LEVEL_CASES)
def test_pcr_heads(b, c, co, d, h, w, m, monkeypatch):
    discipline(monkeypatch, _pcr_level_case(b, c, co, d, h, w, m, norm=False), ["dense2d"] + (["dense3d"] if co else []))


@queries("s2d_pcr_level_workspace_bytes", "s2d_bncm_workspace_bytes", "s2d_pointwise_conv_wgrad_workspace_bytes")
@pytest.mark.parametrize("b,c,co,d,h,w,m", PCR_LEVEL_CASES)
def test_pcr_level(b, c, co, d, h, w, m, monkeypatch):
    discipline(monkeypatch, _pcr_level_case(b, c, co, d, h, w, m, norm=True), ["dense2d", "dense3d"])


# ---- anchor head, NMS -------------------------------------------------------------------------------------------------------------
@queries("s2d_anchor_assign_workspace_bytes", "s2d_anchor_loss_workspace_bytes")
@pytest.mark.parametrize("frames", [(0,), (2,), (0, 1), (2, 0)], ids=str)
def test_anchor_assign_and_loss(frames, golden_dir, monkeypatch):
    """frames of tests/golden/anchor_targets.npz; frame 2 has no boxes (assignment: nothing to match; loss: no positives)"""
    import anchor_util as AU
    from sparse2dense_amd import anchors as A, waymo_configs as WC
    g = np.load(os.path.join(golden_dir, "anchor_targets.npz"))
    sel = list(frames)
    k = max(int((g["classes"][sel] > 0).sum(1).max()), 1)
    boxes = torch.from_numpy(g["boxes"][sel][:, :k].copy()).to(DEV)
    classes = torch.from_numpy(g["classes"][sel][:, :k].copy()).to(DEV)
    table = torch.from_numpy(A.get_assigner(WC.SECOND_ASSIGNER).anchors_numpy([1, AU.H, AU.W])).to(DEV)
    box, cls, dirs = [t.to(DEV) for t in AU.loss_inputs(len(sel))]

    def run():
        out = A.assign_anchor_targets(boxes, classes, WC.SECOND_ASSIGNER)
        labels, targets = out["labels"][0], out["reg_targets"][0]
        leaves = [t.clone().requires_grad_(True) for t in (box, cls, dirs)]
        ret = A.anchor_loss(*leaves, labels, targets, table, AU.LOSS_PARAMS)
        ret["loss"].backward()
        return {"labels": labels, "targets": targets, "weights": out["reg_weights"][0], "loss": [ret[k_] for k_ in A.LOSS_KEYS],
                "elem": ret["loc_loss_elem"], "counts": [ret["num_pos"], ret["num_neg"]], "grads": [t.grad for t in leaves]}
    first = run()
    for i, f in enumerate(frames):   # frame 2 of the fixture is the empty one
        assert (int((first["labels"][i] > 0).sum()) == 0) == (f == 2)
    discipline(monkeypatch, run, ["anchors"])


def _nms_rows(n, seed):
    import test_nms as TN
    boxes = TN._rand_boxes(n, seed)
    scores = np.random.RandomState(seed + 1).uniform(0.05, 1.0, n).astype(np.float32)
    return torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV)


@queries("s2d_nms_workspace_bytes")
@pytest.mark.parametrize("n", [1, 65, 130])
def test_nms(n, monkeypatch):
    from sparse2dense_amd import nms
    boxes, scores = _nms_rows(n, 40 + n)
    run = lambda: {"rotated": nms.rotate_nms(boxes, scores, 0.3, pre_maxsize=4096, post_max_size=500),
                   "circle": nms.circle_nms(boxes[:, :2].contiguous(), scores, 1.5, 83)}
    first = run()
    assert 1 <= first["rotated"].numel() <= n and 1 <= first["circle"].numel() <= n
    discipline(monkeypatch, run, ["nms"])


@queries("s2d_nms_batched_workspace_bytes")
def test_nms_batched(monkeypatch):
    """one call each with the segment counts [0, 1, 65, 130]; every segment equals the one-segment entry on its rows"""
    from sparse2dense_amd import nms
    counts = [0, 1, 65, 130]
    parts = []
    for s, n in enumerate(counts):
        b, sc = _nms_rows(n, 7 + s)
        parts.append(b[torch.sort(sc, descending=True, stable=True)[1]])
    rows = torch.cat(parts)
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    segments = torch.tensor([offs.tolist(), counts], dtype=torch.int32, device=DEV)

    def run():
        keep, n_keep = nms.rotate_nms_batched(rows, segments, counts, 0.3, post_max_size=100)
        ckeep, cn_keep = nms.circle_nms_batched(rows, segments, counts, [1.5] * len(counts), post_max_size=83)
        return {"rotated": [keep[s, :n_keep[s]] for s in range(len(counts))], "n_keep": torch.tensor(n_keep),
                "circle": [ckeep[s, :cn_keep[s]] for s in range(len(counts))], "cn_keep": torch.tensor(cn_keep)}
    first = run()
    assert first["n_keep"][0] == 0 and first["n_keep"][1] == 1 and first["n_keep"][3] > 1
    for s, n in enumerate(counts):
        if n:
            flat_scores = torch.arange(n, 0, -1, device=DEV).float()   # the rows are sorted already
            one = nms.rotate_nms(parts[s], flat_scores, 0.3, post_max_size=100)
            assert torch.equal(one, first["rotated"][s]), s
    discipline(monkeypatch, run, ["nms"])


# ---- deformable convolution -------------------------------------------------------------------------------------------------------
@queries("s2d_deform_conv_bwd_data_workspace_bytes", "s2d_deform_conv_wgrad_workspace_bytes")
@pytest.mark.parametrize("relu", [False, True])
def test_deform_conv_backward(relu, monkeypatch):
    """the enabled 64 -> 64 shape at 2 x 64 x 9 x 13.  y, d_offset, dW: no atomics, bit-identical; dX is accumulated with fp32 atomics
    in the workspace image: all four are held to the bound of tests/test_deform_conv_gpu.py against its float64 composite on every run"""
    import test_deform_conv_gpu as TD
    x, off, wt, dy = TD._operands(2, 9, 13, 3, 7)
    names = ("y", "dX", "d_offset", "dW")
    run = lambda: dict(zip(names, TD._kernel(x, off, wt, dy, relu, torch.float32)))
    first = run()
    mask = (first["y"].double().cpu() > 0).double() if relu else None
    ref = TD._reference(x, off, wt, dy, relu_mask=mask, relu=relu)
    discipline(monkeypatch, run, ["dense2d"], bounded=("dX",),
               check=lambda o: TD._compare([o[k] for k in names], ref, f"workspace discipline relu={relu}"))


# ---- frame preparation, voxelizer, rulebooks --------------------------------------------------------------------------------------
@queries("s2d_prep_workspace_bytes")
@pytest.mark.parametrize("n,m", [(65, 1), (1000, 65), (64, 0), (0, 64)])
def test_compose_clouds(n, m, monkeypatch):
    import frame_prep_util as U
    from sparse2dense_amd import prep
    f = U.random_frame(1, n, m)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pts, boxes, obj = cuda(f["points"]), cuda(f["boxes"]), cuda(f["obj_points"])

    def run():
        dense, recon = prep.compose_clouds(pts, boxes, f["kinds"], obj, f["obj_offsets"])
        return {"dense": dense, "recon": recon, "mask": prep.points_in_rbbox(pts, boxes), "counts": prep.points_count_rbbox(pts, boxes)}
    if m == 0:   # no boxes: nothing is launched, nothing is requested - the wrapper's own early return
        out = run()
        assert out["dense"].shape[0] == n and out["counts"].numel() == 0
        with ws_guard.guard(monkeypatch, 0xFF) as log:
            again = run()
        assert torch.equal(again["dense"], out["dense"]) and torch.equal(again["recon"], out["recon"])
        return
    discipline(monkeypatch, run, ["prep"])


@queries("s2d_voxelize_workspace_bytes")
@pytest.mark.parametrize("name", ["voxelize_small", "voxelize_empty"])
def test_voxelize(name, golden_dir, monkeypatch):
    from sparse2dense_amd import hip_ops as H
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    pts = torch.from_numpy(np.ascontiguousarray(g["points"])).to(DEV)
    run = lambda: {"out": H.voxelize(pts, g["voxel_size"], g["pc_range"], int(g["max_points"]), int(g["max_voxels"]))}
    assert np.array_equal(run()["out"][1].cpu().numpy(), g["coors"])
    discipline(monkeypatch, run, ["hip_ops"])


@queries("s2d_voxelize_batch_workspace_bytes")
@pytest.mark.parametrize("frames", ["all_empty", "mixed"])
def test_voxelize_batch(frames, golden_dir, monkeypatch):
    """all frames empty; and the points of the voxelize_small golden as two frames around an empty one, with the per-frame cut applied"""
    from sparse2dense_amd import hip_ops as H
    g = np.load(os.path.join(golden_dir, "voxelize_small.npz"))
    if frames == "all_empty":
        pts, offs = torch.zeros((0, g["points"].shape[1]), device=DEV), [0, 0, 0]
    else:
        clouds = [g["points"], g["points"][:0], g["points"][::2]]
        pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds, 0))).to(DEV)
        offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist()
    max_voxels = max(int(g["coors"].shape[0]) // 2, 1)
    run = lambda: {"out": H.voxelize_batch(pts, offs, g["voxel_size"], g["pc_range"], int(g["max_points"]), max_voxels)}
    first = run()["out"]
    assert first[4].cpu().tolist() == ([0, 0] if frames == "all_empty" else [max_voxels, 0, first[4][2].item()])
    discipline(monkeypatch, run, ["hip_ops"])


def _rb_tensors(rb):
    return [rb.nbr_out, rb.nbr_in, rb.pair_count, rb.out_coors]


@queries("s2d_rulebook_workspace_bytes")
@pytest.mark.parametrize("occ", [0.03, 0.0])
def test_rulebook(occ, monkeypatch):
    """the smallest grid of tests/test_hip_kernels.py::RB_CASES, SubM and strided, at occupancy 0.03 (three frames), and no rows at all"""
    import test_hip_kernels as TH
    from sparse2dense_amd import hip_ops as H
    shape = (9, 12, 11)
    if occ:
        coors = torch.from_numpy(TH._random_coors(np.random.RandomState(5), 3, shape, occ)).to(DEV)
    else:
        coors = torch.zeros((0, 4), dtype=torch.int32, device=DEV)

    def run():
        subm = H.build_subm_rulebook(coors, 3, shape, (3, 3, 3))
        conv = H.build_conv_rulebook(coors, 3, shape, (3, 3, 3), (2, 2, 2), (1, 1, 1))
        return {"subm": _rb_tensors(subm), "conv": _rb_tensors(conv), "n_out": torch.tensor([subm.n_out, conv.n_out])}
    discipline(monkeypatch, run, ["hip_ops"])


@queries("s2d_rulebook_chain_workspace_bytes")
@pytest.mark.parametrize("n_strided,occ", [(1, 0.03), (2, 0.4)])
def test_rulebook_chain(n_strided, occ, monkeypatch):
    import test_rulebook_chain_gpu as TR
    from sparse2dense_amd import hip_ops as H
    shape, specs = (9, 12, 11), TR.WAYMO_CHAIN[:n_strided]
    assert H.rulebook_chain_supported(3, shape, specs)
    coors = torch.from_numpy(TR._random_coors(np.random.RandomState(9), 3, shape, occ)).to(DEV)

    def run():
        subm, conv = H.build_rulebook_chain(coors, 3, shape, specs, [True] * (n_strided + 1))
        out = {}
        for i, rb in enumerate(subm):
            out[f"subm{i}"] = _rb_tensors(rb)
        for i, rb in enumerate(conv):
            out[f"conv{i}"] = _rb_tensors(rb)
        return out
    discipline(monkeypatch, run, ["hip_ops"])


@queries("s2d_rulebook_sort_workspace_bytes")
@pytest.mark.parametrize("n,kind", [(17, "full"), (1000, "mixed"), (1, "centre")])
def test_rulebook_sort(n, kind, monkeypatch):
    import test_s16_gpu as TS
    from sparse2dense_amd import hip_ops as H
    nbr = TS._shaped_map(n, TS._SHAPES[kind], seed=n, p_drop=0.1 if kind == "mixed" else 0.0)
    discipline(monkeypatch, lambda: {"sorted": H.rulebook_sorted_rows(TS._subm_rulebook(nbr))}, ["hip_ops"])


# ---- optimizer --------------------------------------------------------------------------------------------------------------------
@queries("s2d_grad_norm_workspace_floats")
@pytest.mark.parametrize("scale", [10.0, 0.01], ids=["clips", "does_not_clip"])
def test_grad_norm_and_clip(scale, monkeypatch):
    """tensors of 1, 4095, 4096 and 4097 elements in one table; two steps (the second reuses the cached launch plan)"""
    from sparse2dense_amd.solver import OneCycleAdam
    g = _gen(3)
    shapes = [(1,), (4095,), (4096,), (4097,)]
    params = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * scale for s in shapes] for _ in range(2)]

    def run():
        ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
        opt = OneCycleAdam(ps, wd=0.01, max_grad_norm=35.0)
        norms = []
        for k in range(2):
            for p, gr in zip(ps, grads[k]):
                p.grad = gr.clone().to(DEV)
            norms.append(opt.clip_and_step().clone())
        return {"norms": norms, "params": [p.data for p in ps]}
    first = run()
    ref = torch.linalg.vector_norm(torch.cat([x.flatten() for x in grads[0]]).double())
    np.testing.assert_allclose(float(first["norms"][0]), float(ref), rtol=1e-5)
    discipline(monkeypatch, run, ["solver"])
