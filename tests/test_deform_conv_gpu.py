"""The deformable-convolution kernels (csrc/deform_conv.hip) on the MI355X.

Reference side: sparse2dense_amd.dcn.deform_conv_composite in FLOAT64 on the operands the kernel sees - x, weight and dY rounded to bf16
once and up-cast - run on the host, or (workload shape) through torch's own float64 device kernels.  Never an s2d kernel.

Offsets are integers in [-8 r, 8 r] divided by 8: exact in fp32 and bf16, so every position and bilinear weight is exact in fp32, no
floor can fall differently on the two sides, and integer positions, the -1 / H window edges and out-of-range taps occur by
construction.  Every comparison is over whole tensors.

Tolerance: the project's bf16 criterion of tests/test_dense2d_gpu.py, max|err| <= 6e-3 * max|ref| per tensor, for y, dX, d_offset, dW.

Fused ReLU: the kernel's backward re-derives the mask from its saved bf16 output.  The sampled values are stored as bf16 in LDS (2^-9
relative each), so the sign of an output within that rounding of zero can differ from the float64 one, and ONE such mask entry moves a
gradient by a whole term W * dY against sums whose maximum is ~50 terms: the float64 composite with nothing but its sampled columns
rounded to bf16 already misses 6e-3 by a factor of ten that way (tests/test_deform_conv_cpu.py::
test_relu_sign_flips_of_bf16_storage_alone_exceed_the_gradient_tolerance holds the figures).  That is a property of bf16 storage in
front of a ReLU, not of a kernel, so the mask is an operand like the others: the reference backward runs with the mask the kernel sees
(saved output > 0).  The mask itself is pinned by the forward comparison, which is against relu(float64) without it - an output with
the wrong sign by more than the tolerance fails there - and by a bound of 2e-3 on the fraction of signs that differ."""
import pytest
import torch
import torch.nn.functional as F

from sparse2dense_amd import _lib, dcn, dense2d, heads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 6e-3
GEO = (64, 3, 3, 1, 1, 1, 4)   # cout, kh, kw, stride, pad, dil, dg


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _operands(n, h, w, r, seed, cin=64, cout=64, dg=4):
    """bf16-exact x, weight, dY and 1/8-grid offsets, as float64 host tensors"""
    g = _gen(seed)
    x = torch.randn(n, cin, h, w, generator=g).bfloat16().double()
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).bfloat16().double()
    off = torch.randint(-8 * r, 8 * r + 1, (n, dg * 18, h, w), generator=g).double() / 8 if r else torch.zeros(n, dg * 18, h, w, dtype=torch.float64)
    dy = torch.randn(n, cout, h, w, generator=g).bfloat16().double()
    return x, off, wt, dy


def _reference(x, off, wt, dy, relu_mask=None, relu=False, dg=4):
    """float64 composite: y, dX, d_offset, dW.  relu: y = relu(.); relu_mask: the mask of the backward (see the module docstring)"""
    xx, oo, ww = (t.clone().requires_grad_(True) for t in (x, off, wt))
    y0 = dcn.deform_conv_composite(xx, oo, ww, 1, 1, 1, 1, dg)
    y = torch.relu(y0) if relu else y0
    yb = y0 * relu_mask if relu_mask is not None else y
    gx, go, gw = torch.autograd.grad((yb * dy).sum(), (xx, oo, ww))
    return y.detach(), gx, go, gw


def _kernel(x, off, wt, dy, relu, off_dtype, dev=DEV):
    """the three entry points on device copies -> y, dX, d_offset, dW (device tensors)"""
    xb = x.to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    ob = off.to(dev).to(off_dtype).contiguous(memory_format=torch.channels_last)
    dyb = dy.to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    wd = wt.to(dev).float().contiguous()
    pf, pb = dcn.pack_weights(wd)
    y = dcn.deform_conv_fwd_hip(xb, ob, pf, *GEO, relu)
    ys = y if relu else None
    dx, doff = dcn.deform_conv_bwd_data_hip(xb, ob, dyb, ys, pb, *GEO)
    dw = dcn.deform_conv_wgrad_hip(xb, ob, dyb, ys, *GEO)
    assert doff.dtype == off_dtype and dx.dtype == torch.bfloat16 and dw.dtype == torch.float32
    return y, dx, doff, dw


def _compare(got, ref, what):
    worst = {}
    for name, a, b in zip(("y", "dX", "d_offset", "dW"), got, ref):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        assert a.shape == b.shape, (name, a.shape, b.shape)
        assert torch.isfinite(a).all(), name
        worst[name] = float((a - b).abs().max() / b.abs().max())
    print(what, {k: f"{v:.2e}" for k, v in worst.items()})
    for name, v in worst.items():
        assert v <= TOL, (what, name, v)


def _check(shape, r, seed, relu, off_dtype):
    x, off, wt, dy = _operands(*shape, r, seed)
    got = _kernel(x, off, wt, dy, relu, off_dtype)
    mask = (got[0].double().cpu() > 0).double() if relu else None
    ref = _reference(x, off, wt, dy, relu_mask=mask, relu=relu)
    if relu:
        disagree = float(((ref[0] > 0).double() != mask).double().mean())
        assert disagree <= 2e-3, disagree   # (measured on the host emulation: 5e-4)
    _compare(got, ref, f"{shape} r={r} relu={relu} {off_dtype}")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("off_dtype", [torch.float32, torch.bfloat16])
def test_odd_extents_and_taps_outside_the_map(relu, off_dtype):
    """2 x 64 x 13 x 11, r = 5: 143 pixels per image is a multiple of no tile size, a third of the taps lie outside"""
    _check((2, 13, 11), 5, 1, relu, off_dtype)


def test_several_workgroups_and_a_ragged_last_tile():
    _check((1, 37, 29), 2, 2, True, torch.float32)


def test_zero_offsets_equal_the_plain_convolution():
    x, off, wt, dy = _operands(3, 16, 16, 0, 3)
    got = _kernel(x, off, wt, dy, False, torch.float32)
    ref = F.conv2d(x, wt, padding=1)
    err = float((got[0].double().cpu() - ref).abs().max() / ref.abs().max())
    xb = x.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    dense = dense2d.conv3x3_nhwc(xb, dense2d.pack_weights(wt.to(DEV).float()), None, 64, 64, 1)
    err_dense = float((got[0].double() - dense.double()).abs().max().cpu() / ref.abs().max())
    print("zero offsets: vs float64 conv2d", f"{err:.2e}", "vs conv3x3_nhwc", f"{err_dense:.2e}")
    assert err <= TOL and err_dense <= TOL
    _compare(got, _reference(x, off, wt, dy), "zero offsets")


def test_workload_shape_against_the_float64_composite_on_the_device():
    """2 x 64 x 180 x 180 (the nuScenes 0.075 m map), r = 3: the size tools/deform_conv_bench.py times"""
    x, off, wt, dy = _operands(2, 180, 180, 3, 4)
    got = _kernel(x, off, wt, dy, True, torch.bfloat16)
    mask = (got[0] > 0).double()
    ref = _reference(x.to(DEV), off.to(DEV), wt.to(DEV), dy.to(DEV), relu_mask=mask, relu=True)
    assert float(((ref[0] > 0).double() != mask).double().mean()) <= 2e-3
    _compare(got, ref, "workload shape")


def _banded(shape_nchw, dtype, fill, band=4096):
    """a channels_last [n, c, h, w] view in the middle of a larger sentinel-filled buffer -> (view, whole buffer)"""
    n, c, h, w = shape_nchw
    buf = torch.full((2 * band + n * h * w * c,), fill, dtype=dtype, device=DEV)
    view = buf[band:band + n * h * w * c].view(n, h, w, c).permute(0, 3, 1, 2)
    assert view.is_contiguous(memory_format=torch.channels_last)
    return view, buf


def test_hostile_offsets_stay_inside_the_buffers():
    """+-1e6, NaN and +-Inf offsets: the forward and both backwards return, every output whose taps are all finite equals the reference,
    and 4096-element guard bands around x, y, dX, d_offset and the fp32 image that the data backward's atomics scatter into (the
    write whose address comes from an offset) keep their sentinel: masking happens before addressing."""
    n, h, w, band = 2, 13, 11, 4096
    x, off, wt, dy = _operands(n, h, w, 2, 5)
    g = _gen(6)
    kind = torch.randint(0, 2000, off.shape, generator=g)   # ~50 hostile values, 5 of 6 pixels keep finite taps
    for code, val in ((0, 1e6), (1, -1e6), (2, float("nan")), (3, float("inf")), (4, float("-inf"))):
        assert int((kind == code).sum()) > 0
        off[kind == code] = val
    finite_px = torch.isfinite(off).all(1, keepdim=True)                    # [n, 1, h, w]: pixels whose taps are all finite
    assert 0.5 < float(finite_px.double().mean()) < 0.95
    ref_off = torch.where(torch.isfinite(off), off, torch.full_like(off, 1e6))   # a non-finite position samples nothing, like one far outside
    ref = _reference(x, ref_off, wt, dy)
    xv, xbuf = _banded((n, 64, h, w), torch.bfloat16, 7.0)
    xv.copy_(x.to(DEV))
    yv, ybuf = _banded((n, 64, h, w), torch.bfloat16, 7.0)
    dxv, dxbuf = _banded((n, 64, h, w), torch.bfloat16, 7.0)
    dov, dobuf = _banded((n, 72, h, w), torch.float32, 7.0)
    ob = off.to(DEV).float().contiguous(memory_format=torch.channels_last)
    dyb = dy.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    pf, pb = dcn.pack_weights(wt.to(DEV).float().contiguous())
    dcn.deform_conv_fwd_hip(xv, ob, pf, *GEO, False, y=yv)
    ws_bytes = _lib.load().s2d_deform_conv_bwd_data_workspace_bytes(n, h, w, 64)
    assert ws_bytes == n * h * w * 64 * 4
    wsbuf = torch.full((2 * band + ws_bytes // 4,), 7.0, dtype=torch.float32, device=DEV)
    ws = wsbuf[band:band + ws_bytes // 4].view(torch.uint8)
    dcn.deform_conv_bwd_data_hip(xv, ob, dyb, None, pb, *GEO, dx=dxv, d_offset=dov, ws=ws)
    dw = dcn.deform_conv_wgrad_hip(xv, ob, dyb, None, *GEO)
    torch.cuda.synchronize()
    for name, buf, numel in (("x", xbuf, xv.numel()), ("y", ybuf, yv.numel()), ("dX", dxbuf, dxv.numel()), ("d_offset", dobuf, dov.numel()),
                             ("fp32 dX image", wsbuf, ws_bytes // 4)):
        assert bool((buf[:band] == 7.0).all()) and bool((buf[band + numel:] == 7.0).all()), f"guard band of {name} was written"
    assert torch.equal(xv.cpu().double(), x)
    assert torch.equal(wsbuf[band:band + ws_bytes // 4].view(n, h, w, 64).permute(0, 3, 1, 2).bfloat16(), dxv)   # dX is that image, rounded once
    y, dx, doff = yv.double().cpu(), dxv.double().cpu(), dov.double().cpu()
    for name, a, b, m in (("y", y, ref[0], finite_px), ("d_offset", doff, ref[2], finite_px)):
        err = float(((a - b).abs() * m).max() / b.abs().max())
        print("hostile", name, f"{err:.2e}")
        assert torch.isfinite(a[m.expand_as(a)]).all() and err <= TOL, (name, err)
    # the kernel treats a non-finite position as outside the window, so the sums over all pixels agree as well
    _compare((y, dx, doff, dw), ref, "hostile offsets, whole tensors")


def test_outputs_without_atomics_are_bit_identical_from_run_to_run():
    x, off, wt, dy = _operands(2, 37, 29, 3, 7)
    a = _kernel(x, off, wt, dy, True, torch.float32)
    b = _kernel(x, off, wt, dy, True, torch.float32)
    for name, i in (("y", 0), ("d_offset", 2), ("dW", 3)):
        assert torch.equal(a[i], b[i]), name
    scale = float(a[1].double().abs().max())
    assert float((a[1].double() - b[1].double()).abs().max()) <= TOL * scale   # dX: fp32 atomics in any order, then one bf16 rounding


def test_library_loader_and_the_composite_for_uncovered_shapes():
    lib = _lib.load()
    assert lib.s2d_deform_conv_supported(64, 64, 3, 3, 1, 1, 1, 1, 4) == 1
    assert lib.s2d_deform_conv_supported(64, 64, 3, 3, 1, 1, 1, 2, 4) == 0    # groups = 2
    assert lib.s2d_deform_conv_supported(48, 64, 3, 3, 1, 1, 1, 1, 3) == 0    # Cin = 48
    assert lib.s2d_deform_conv_supported(64, 64, 5, 5, 1, 2, 1, 1, 4) == 0    # a 5 x 5 kernel
    for other in ((128, 64, 3, 3, 1, 1, 1, 1, 4), (64, 128, 3, 3, 1, 1, 1, 1, 4), (64, 64, 3, 3, 2, 1, 1, 1, 4), (64, 64, 3, 3, 1, 0, 1, 1, 4),
                  (64, 64, 3, 3, 1, 2, 2, 1, 4), (64, 64, 3, 3, 1, 1, 1, 1, 2), (64, 64, 3, 3, 1, 1, 1, 1, 1)):
        assert lib.s2d_deform_conv_supported(*other) == 0, other               # enabled = what this file runs the kernels at, nothing wider
    assert lib.s2d_deform_conv_workspace_bytes(2, 180, 180, 64, 64, 3, 3) == 0
    assert lib.s2d_deform_conv_wgrad_workspace_bytes(2, 180, 180, 64, 64, 3, 3, 1, 1, 1) > 0
    g = _gen(8)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for cin, cout, k, groups, dg in ((64, 64, 3, 2, 4), (48, 64, 3, 1, 3), (64, 64, 5, 1, 4)):
            x = torch.randn(1, cin, 10, 9, generator=g).to(DEV)
            wt = (torch.randn(cout, cin // groups, k, k, generator=g) / 24).to(DEV)
            off = (torch.randint(-16, 17, (1, dg * 2 * k * k, 10, 9), generator=g).float() / 8).to(DEV)
            assert not dcn._hip_ok(x, off, wt, (1, 1), (k // 2, k // 2), (1, 1), groups, dg)
            y = dcn.deform_conv(x, off, wt, 1, k // 2, 1, groups, dg)
            ref = dcn.deform_conv_composite(x.double(), off.double(), wt.double(), 1, k // 2, 1, groups, dg)
            assert float((y.double() - ref).abs().max() / ref.abs().max()) <= 2e-2   # (the composite's einsum runs in bf16 under autocast)
        x = torch.randn(1, 64, 10, 9, generator=g).to(DEV)
        wt = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(DEV)
        off = torch.zeros(1, 72, 10, 9, device=DEV)
        assert dcn._hip_ok(x, off, wt, (1, 1), (1, 1), (1, 1), 1, 4)
    assert not dcn._hip_ok(x, off, wt, (1, 1), (1, 1), (1, 1), 1, 4)   # fp32 "reference precision" mode: the composite


# ---- module level ------------------------------------------------------------------------------------------------------------------
class _KernelOperands:
    """Makes the float64 composite module run on the operands the kernel saw: the offsets the product's conv_offset produced (bf16 on
    the device; a float64 conv_offset differs by their rounding, and a position that crosses an integer changes the corner set) and the
    ReLU mask of the product's saved output.  Values are substituted, gradients flow to the reference module's own layers.
    The batch norms with a fused ReLU behind the deformable convs are treated the same way (`record_bn` / `replay_bn`): their masks
    come from the product's stored bf16 output, for the reason the module docstring gives for the deformable conv's own ReLU.
    `dz_abs` holds, per conv of the reference, the per-channel sum of |gradient| at its output (see `_zero_gradient_bound`)."""

    def __init__(self):
        self.offsets, self.outputs, self.ref_outputs = [], [], []
        self.bn_masks, self.dz_abs = {}, {}

    def record_bn(self, mod):
        from sparse2dense_amd.dense2d import FastBatchNorm2d
        for name, m in mod.named_modules():
            if isinstance(m, FastBatchNorm2d) and m.fused_relu == 1:
                m.register_forward_hook(lambda _m, _i, o, name=name: self.bn_masks.__setitem__(name, (o.detach() > 0).double().cpu()))

    def replay_bn(self, ref):
        from sparse2dense_amd.dense2d import FastBatchNorm2d
        for name, m in ref.named_modules():
            if isinstance(m, FastBatchNorm2d) and m.fused_relu == 1:
                m.forward = lambda x, m=m, name=name: torch.nn.BatchNorm2d.forward(m, x) * self.bn_masks[name]
            if isinstance(m, torch.nn.Conv2d):
                def hook(_m, _i, o, name=name):
                    if o.requires_grad:
                        o.register_hook(lambda g: self.dz_abs.__setitem__(name, g.detach().abs().sum((0, 2, 3))))
                m.register_forward_hook(hook)

    def record(self, fa):
        fa.conv_offset.register_forward_hook(lambda m, i, o: self.offsets.append(o.detach().double().cpu()))
        fa.conv_adaption.register_forward_hook(lambda m, i, o: self.outputs.append(o.detach().double().cpu()))

    def replay(self, fa, idx):
        """idx: position of this FeatureAdaption in the module's call order"""
        def forward(x):
            o = fa.conv_offset(x)
            o = o + (self.offsets[idx] - o).detach()
            y0 = dcn.deform_conv_composite(x, o, fa.conv_adaption.weight, 1, 1, 1, 1, 4)
            self.ref_outputs.append(torch.relu(y0).detach())
            return y0 * (self.outputs[idx] > 0).double()
        fa.forward = forward


def _bf16_params(m):
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.bfloat16().float())
    return m


def _run_pair(make, x, coherent_seed):
    """`make()` -> module; runs it in bf16 mode on the kernels and as a float64 composite copy on the same operands.
    -> (outputs, gradients) of both sides as dicts of host float64 tensors"""
    import copy
    torch.manual_seed(0)
    mod = _bf16_params(make()).train()
    ref = copy.deepcopy(mod).double()
    fas = lambda m: [s for s in m.modules() if isinstance(s, heads.FeatureAdaption)]
    rec = _KernelOperands()
    mod = mod.to(DEV)
    for m in mod.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.to(memory_format=torch.channels_last)
    for fa in fas(mod):
        rec.record(fa)
    rec.record_bn(mod)
    xg = x.to(DEV).float().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for fa in fas(mod):
            probe = xg.detach().bfloat16()
            assert dcn._hip_ok(probe, fa.conv_offset(probe), fa.conv_adaption.weight, (1, 1), (1, 1), (1, 1), 1, 4)
        rec.offsets.clear()
        out = mod(xg)
    out = out if isinstance(out, dict) else {"y": out}
    wts = {k: (torch.randn(v.shape, generator=_gen(coherent_seed + i)).abs() + 0.5) for i, (k, v) in enumerate(sorted(out.items()))}
    loss = sum((out[k].float() * wts[k].to(DEV)).sum() for k in out)
    names = [n for n, _ in mod.named_parameters()]
    grads = torch.autograd.grad(loss, [xg] + [p for _, p in mod.named_parameters()])
    torch.cuda.synchronize()
    got = ({k: v.detach().double().cpu() for k, v in out.items()}, {n: g.double().cpu() for n, g in zip(["x"] + names, grads)})
    # the same module through the composite in float64 (host), bf16-rounded parameters, the kernel's offsets and ReLU masks
    for idx, fa in enumerate(fas(ref)):
        rec.replay(fa, idx)
    rec.replay_bn(ref)
    xr = x.double().requires_grad_(True)
    outr = ref(xr)
    outr = outr if isinstance(outr, dict) else {"y": outr}
    lossr = sum((outr[k] * wts[k].double()).sum() for k in outr)
    gradsr = torch.autograd.grad(lossr, [xr] + [p for _, p in ref.named_parameters()])
    want = ({k: v.detach() for k, v in outr.items()}, dict(zip(["x"] + names, gradsr)))
    assert len(rec.outputs) == len(rec.ref_outputs) == len(fas(ref))
    for i, (a, b) in enumerate(zip(rec.outputs, rec.ref_outputs)):   # the deformable conv's own output (in front of every batch norm): 6e-3 of max
        err = _max_err(a, b)
        print("feature adaption", i, "output", f"{err:.2e}")
        assert err <= TOL, (i, err)
    got[1]["_dz_abs"] = rec.dz_abs
    return got, want


def _zero_gradient_bound(name, g, dz_abs):
    """The bias of a conv in front of a train-mode batch norm has the EXACT gradient zero (the batch norm's backward removes the
    per-channel mean of dz), so no relative error exists.  The product sums dz as stored, in bf16: every element carries a rounding of
    at most half an ulp, 2^-9 relative, so |sum| <= 2^-9 * sum |dz| per channel; one more factor of two for the bf16 rounding of the
    result's own inputs in the batch-norm backward kernel: 2^-8 * sum |dz| (the reference's dz)."""
    bound = dz_abs[name.rsplit(".", 1)[0]] * 2.0 ** -8
    assert bool((g.abs() <= bound).all()), (name, float((g.abs() / bound).max()))


def _max_err(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _feature_adaption():
    fa = heads.FeatureAdaption(64, 64)
    torch.nn.init.normal_(fa.conv_offset.weight, std=0.15)   # offsets of a few pixels (the zero initialisation would test one corner only)
    return fa


def test_feature_adaption_module_matches_the_float64_composite():
    x = torch.randn(2, 64, 20, 24, generator=_gen(9)).bfloat16()
    (out, grads), (outr, gradsr) = _run_pair(_feature_adaption, x, 100)
    grads.pop("_dz_abs")
    errs = {"y": _max_err(out["y"], outr["y"])}
    errs.update({n: _max_err(grads[n], gradsr[n]) for n in grads})
    print("FeatureAdaption", {k: f"{v:.2e}" for k, v in errs.items()})
    assert set(grads) == {"x", "conv_offset.weight", "conv_offset.bias", "conv_adaption.weight"}
    for n, v in errs.items():   # the deformable conv's own tensors: 6e-3 of max
        assert v <= TOL, (n, v)


def test_dcn_sep_head_module_matches_the_float64_composite():
    """Outputs and gradients behind the batch norms: the norm-wise 5e-2 of the bf16 CenterHead test (tests/test_dense_modules.py:298,
    `_run_head(golden_dir, "cuda:0", 5e-2, 0, bf16=True)`).  The reference runs on the operands the kernels saw, the ReLU masks of the
    fused batch norms included (_KernelOperands): a sign that differs within bf16 rounding of zero moves these gradients beyond the bound
    by itself, as the module docstring explains for the deformable conv's own ReLU.  The biases of the six convs in front of a
    train-mode batch norm have the exact gradient zero and get an absolute bound: see _zero_gradient_bound."""
    from golden_util import rel_err
    common = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}

    def make():
        h = heads.DCNSepHead(64, 2, dict(common), bn=True, init_bias=-2.19, final_kernel=3)
        for fa in (h.feature_adapt_cls, h.feature_adapt_reg):
            torch.nn.init.normal_(fa.conv_offset.weight, std=0.15)
        return h
    x = torch.randn(2, 64, 20, 24, generator=_gen(10)).bfloat16()
    (out, grads), (outr, gradsr) = _run_pair(make, x, 200)
    dz_abs = grads.pop("_dz_abs")
    assert set(out) == set(common) | {"hm"} and set(out) == set(outr)
    for k, (c, _) in dict(common, hm=(2, 2)).items():
        assert tuple(out[k].shape) == (2, c, 20, 24), k
    errs = {k: rel_err(out[k], outr[k]) for k in out}
    exact_zero = [n for n in grads if n.endswith(".0.bias") and float(gradsr[n].norm()) <= 1e-12 * float(gradsr[n[:-4] + "weight"].norm())]
    assert len(exact_zero) == 6, exact_zero   # cls_head.0 and the five task_head.<head>.0: convs in front of a train-mode batch norm
    for n in exact_zero:
        _zero_gradient_bound(n, grads[n], dz_abs)
    gerrs = {n: rel_err(grads[n], gradsr[n]) for n in grads if n not in exact_zero}
    print("DCNSepHead outputs", {k: f"{v:.1e}" for k, v in errs.items()})
    print("DCNSepHead worst gradients", sorted(((f"{v:.1e}", n) for n, v in gerrs.items()), reverse=True)[:6])
    assert len(gerrs) + len(exact_zero) == 1 + len(list(make().parameters()))
    assert max(errs.values()) <= 5e-2, errs
    assert max(gerrs.values()) <= 5e-2, gerrs
