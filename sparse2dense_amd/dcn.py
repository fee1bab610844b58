"""Deformable convolution v1 (det3d/ops/dcn/deform_conv.py: DeformConvFunction, deform_conv, DeformConv).

`DeformConv` keeps the reference's constructor signature, attributes, its single `weight` parameter and its initialisation, so the
nuScenes DCN configs (CenterHead(dcn_head=True), bbox_heads/center_head.py:25-63) and their checkpoints load unchanged.

Two paths:
  * HIP (csrc/deform_conv.hip): CUDA tensors under bf16 autocast for the shapes `s2d_deform_conv_supported` names - a fused implicit
    GEMM per call (no column buffer), data gradient on the chain, weight gradient through side.run like the other dense convs.
  * composite: corner gathers + einsum in plain torch, differentiable by autograd in any dtype including float64.  It serves CPU tensors
    (the reference raises there), the fp32 "reference precision" mode and the shapes the kernel does not cover - nothing more.

Out of scope and absent on purpose (no config of the reference tree uses them): ModulatedDeformConv / ModulatedDeformConvPack /
DeformConvPack (the v2 form and the self-contained offset convs) and the deformable PSROI pooling (DeformRoIPooling*).
"""
import math

import torch
from torch import nn
import torch.nn.functional as F
from torch.nn.modules.utils import _pair, _single

from . import _lib
from . import side as _side
from ._lib import check

ENABLED = True   # tools / tests can switch the kernel off to A/B against the composite


def _out_size(h, w, kh, kw, stride, padding, dilation):
    ho = (h + 2 * padding[0] - (dilation[0] * (kh - 1) + 1)) // stride[0] + 1
    wo = (w + 2 * padding[1] - (dilation[1] * (kw - 1) + 1)) // stride[1] + 1
    if ho <= 0 or wo <= 0:
        raise ValueError(f"convolution input is too small (output would be {ho}x{wo})")
    return ho, wo


def deform_conv_composite(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1):
    """The definition in plain torch ops.  Position h = ho*stride - pad + i*dil + off_h; the sample is 0 unless
    h > -1 and w > -1 and h < H and w < W (strict), else the bilinear blend over floor / floor + 1 with every corner counted only inside
    [0, H-1] x [0, W-1].  floor has no gradient, so the offset gradient at an integer position is the right-hand derivative."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    n, c, h, w = input.shape
    cout, cin_g, kh, kw = weight.shape
    dg, k = deformable_groups, kh * kw
    assert c % dg == 0 and c == cin_g * groups and cout % groups == 0
    ho, wo = _out_size(h, w, kh, kw, stride, padding, dilation)
    assert tuple(offset.shape) == (n, dg * 2 * k, ho, wo), (tuple(offset.shape), (n, dg * 2 * k, ho, wo))
    dt = torch.promote_types(torch.promote_types(input.dtype, weight.dtype), offset.dtype)
    x, off, wt = input.to(dt), offset.to(dt), weight.to(dt)
    dev = x.device
    off = off.reshape(n, dg, k, 2, ho, wo)
    ti = torch.arange(kh, device=dev).repeat_interleave(kw) * dilation[0]
    tj = torch.arange(kw, device=dev).repeat(kh) * dilation[1]
    base_h = (torch.arange(ho, device=dev) * stride[0] - padding[0])[None, :, None] + ti[:, None, None]   # [k, ho, 1]
    base_w = (torch.arange(wo, device=dev) * stride[1] - padding[1])[None, None, :] + tj[:, None, None]   # [k, 1, wo]
    ph = base_h.to(dt) + off[:, :, :, 0]   # [n, dg, k, ho, wo]
    pw = base_w.to(dt) + off[:, :, :, 1]
    inside = (ph > -1) & (pw > -1) & (ph < h) & (pw < w)   # False for NaN
    ph = torch.where(inside, ph, torch.zeros_like(ph))
    pw = torch.where(inside, pw, torch.zeros_like(pw))
    fh, fw = torch.floor(ph).detach(), torch.floor(pw).detach()
    lh, lw = ph - fh, pw - fw
    hl, wl = fh.long(), fw.long()
    xg = x.reshape(n, dg, c // dg, h * w)
    col = None
    for dy, dx, cw in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        yy, xx = hl + dy, wl + dx
        ok = inside & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(n, dg, 1, k * ho * wo).expand(-1, -1, c // dg, -1)
        term = torch.gather(xg, 3, idx) * (cw * ok.to(dt)).reshape(n, dg, 1, k * ho * wo)
        col = term if col is None else col + term
    col = col.reshape(n, groups, cin_g, k, ho * wo)
    out = torch.einsum("gock,ngckl->ngol", wt.reshape(groups, cout // groups, cin_g, k), col)
    return out.reshape(n, cout, ho, wo)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _nhwc_bf16(t):
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _nhwc_offset(t):
    """fp32 or bf16, channels_last: a tensor that already is goes through untouched (no layout copy)"""
    if t.dtype not in (torch.float32, torch.bfloat16):
        t = t.float()
    return t.contiguous(memory_format=torch.channels_last)


def supported(cin, cout, kh, kw, stride, padding, dilation, groups, dg):
    sq = stride[0] == stride[1] and padding[0] == padding[1] and dilation[0] == dilation[1]
    return bool(sq and _lib.load().s2d_deform_conv_supported(int(cin), int(cout), int(kh), int(kw), int(stride[0]), int(padding[0]),
                                                              int(dilation[0]), int(groups), int(dg)))


def pack_weights(weight):
    """fp32 [cout][cin][kh][kw] -> (forward image, data-gradient image), both bf16, one launch; cached per parameter version"""
    from . import dense2d as D

    def build():
        lib = _lib.load()
        cout, cin, kh, kw = weight.shape
        w = weight.detach()
        if w.dtype != torch.float32 or not w.is_contiguous():
            w = w.float().contiguous()
        pf = torch.empty(kh * kw * cin * cout, dtype=torch.bfloat16, device=weight.device)
        pb = torch.empty_like(pf)
        launch = lambda: check(lib.s2d_deform_conv_pack_weights_bf16(_ptr(w), cin, cout, kh, kw, _ptr(pf), _ptr(pb), _stream()),
                               "s2d_deform_conv_pack_weights_bf16")
        launch()
        D.register_repack(weight, [("deform_conv",)], w, launch)
        return pf, pb
    return D.cached_pack(weight, ("deform_conv",), build)


def deform_conv_fwd_hip(xb, ob, packed_fwd, cout, kh, kw, stride, pad, dil, dg, relu, y=None):
    """xb bf16 NHWC, ob fp32 / bf16 NHWC -> y bf16 NHWC; ONE kernel launch, no workspace"""
    lib = _lib.load()
    n, cin, h, w = xb.shape
    ho, wo = _out_size(h, w, kh, kw, (stride, stride), (pad, pad), (dil, dil))
    assert xb.dtype == torch.bfloat16 and xb.is_contiguous(memory_format=torch.channels_last)
    assert ob.is_contiguous(memory_format=torch.channels_last) and tuple(ob.shape) == (n, dg * 2 * kh * kw, ho, wo)
    if y is None:
        y = torch.empty((n, cout, ho, wo), dtype=torch.bfloat16, device=xb.device, memory_format=torch.channels_last)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (n, cout, ho, wo) and y.is_contiguous(memory_format=torch.channels_last)
    check(lib.s2d_deform_conv_nhwc_bf16(_ptr(xb), _ptr(ob), int(ob.dtype == torch.bfloat16), _ptr(packed_fwd), n, h, w, cin, cout, kh, kw, stride, pad,
                                        dil, dg, int(bool(relu)), _ptr(y), _stream()), "s2d_deform_conv_nhwc_bf16")
    return y


def deform_conv_bwd_data_hip(xb, ob, dyb, y_saved, packed_bwd, cout, kh, kw, stride, pad, dil, dg, dx=None, d_offset=None, ws=None):
    """-> (dx bf16 NHWC, d_offset in ob's dtype and layout); y_saved: the forward's output when its ReLU was fused, else None;
    ws: a caller-owned uint8 workspace of s2d_deform_conv_bwd_data_workspace_bytes (the fp32 image the atomics accumulate into)"""
    from .dense2d import _ws
    lib = _lib.load()
    n, cin, h, w = xb.shape
    assert dyb.dtype == torch.bfloat16 and dyb.is_contiguous(memory_format=torch.channels_last) and dyb.shape[1] == cout
    dx = torch.empty_like(xb) if dx is None else dx
    d_offset = torch.empty_like(ob) if d_offset is None else d_offset
    if ws is None:
        ws = _ws(lib.s2d_deform_conv_bwd_data_workspace_bytes(n, h, w, cin), xb.device)
    check(lib.s2d_deform_conv_bwd_data_nhwc_bf16(_ptr(xb), _ptr(ob), int(ob.dtype == torch.bfloat16), _ptr(dyb), _ptr(y_saved), _ptr(packed_bwd), n, h, w,
                                                 cin, cout, kh, kw, stride, pad, dil, dg, _ptr(dx), _ptr(d_offset), _ptr(ws), ws.numel(), _stream()),
          "s2d_deform_conv_bwd_data_nhwc_bf16")
    return dx, d_offset


def deform_conv_wgrad_hip(xb, ob, dyb, y_saved, cout, kh, kw, stride, pad, dil, dg):
    """-> dweight fp32 [cout][cin][kh][kw]; deterministic"""
    from .dense2d import _ws
    lib = _lib.load()
    n, cin, h, w = xb.shape
    dw = torch.empty((cout, cin, kh, kw), dtype=torch.float32, device=xb.device)
    ws = _ws(lib.s2d_deform_conv_wgrad_workspace_bytes(n, h, w, cin, cout, kh, kw, stride, pad, dil), xb.device)
    check(lib.s2d_deform_conv_wgrad_nhwc_bf16(_ptr(xb), _ptr(ob), int(ob.dtype == torch.bfloat16), _ptr(dyb), _ptr(y_saved), n, h, w, cin, cout, kh, kw,
                                              stride, pad, dil, dg, _ptr(dw), _ptr(ws), ws.numel(), _stream()), "s2d_deform_conv_wgrad_nhwc_bf16")
    return dw


class _DeformConvHipFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offset, weight, stride, pad, dil, dg, relu):
        xb, ob = _nhwc_bf16(x), _nhwc_offset(offset)
        cout, _, kh, kw = weight.shape
        pf, _ = pack_weights(weight)
        y = deform_conv_fwd_hip(xb, ob, pf, cout, kh, kw, stride, pad, dil, dg, relu)
        ctx.save_for_backward(xb, ob, weight, y if relu else None)
        ctx.geo = (cout, kh, kw, stride, pad, dil, dg)
        ctx.off_dtype = offset.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        xb, ob, weight, y_saved = ctx.saved_tensors
        dyb = _nhwc_bf16(dy)
        dx = doff = dw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:   # on the chain: the layers below wait for these
            dx, doff = deform_conv_bwd_data_hip(xb, ob, dyb, y_saved, pack_weights(weight)[1], *ctx.geo)
            doff = doff.to(ctx.off_dtype)
        if ctx.needs_input_grad[2]:   # off the chain: second stream when enabled (side.py)
            dw = _side.run(weight, lambda: deform_conv_wgrad_hip(xb, ob, dyb, y_saved, *ctx.geo).to(weight.dtype), xb, ob, dyb, y_saved)
        return dx, doff, _side.undefer(dw), None, None, None, None, None


def _hip_ok(input, offset, weight, stride, padding, dilation, groups, dg):
    return (ENABLED and input.is_cuda and offset.is_cuda and input.dim() == 4 and torch.is_autocast_enabled()
            and torch.get_autocast_gpu_dtype() == torch.bfloat16
            and supported(weight.shape[1] * groups, weight.shape[0], weight.shape[2], weight.shape[3], stride, padding, dilation, groups, dg))


def _deform_conv(input, offset, weight, stride, padding, dilation, groups, deformable_groups, relu):
    if input is not None and input.dim() != 4:
        raise ValueError(f"Expected 4D tensor as input, got {input.dim()}D tensor instead.")
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    if _hip_ok(input, offset, weight, stride, padding, dilation, groups, deformable_groups):
        return _DeformConvHipFn.apply(input, offset, weight, stride[0], padding[0], dilation[0], deformable_groups, relu)
    out = deform_conv_composite(input, offset, weight, stride, padding, dilation, groups, deformable_groups)
    return F.relu(out) if relu else out


def deform_conv(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, im2col_step=64):
    """The reference's functional form.  im2col_step changes no value (it only splits the reference's column buffer) and is ignored."""
    return _deform_conv(input, offset, weight, stride, padding, dilation, groups, deformable_groups, False)


class DeformConvFunction:
    """call-site compatibility: the reference's `DeformConvFunction.apply(input, offset, weight, ...)`"""
    apply = staticmethod(deform_conv)

    @staticmethod
    def _output_size(input, weight, padding, dilation, stride):
        ho, wo = _out_size(input.size(2), input.size(3), weight.size(2), weight.size(3), _pair(stride), _pair(padding), _pair(dilation))
        return (input.size(0), weight.size(0), ho, wo)


class DeformConv(nn.Module):
    fused_relu = False   # set by FeatureAdaption: the ReLU behind this layer runs in the kernel's epilogue

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=False):
        super().__init__()
        assert not bias
        assert in_channels % groups == 0, f"in_channels {in_channels} cannot be divisible by groups {groups}"
        assert out_channels % groups == 0, f"out_channels {out_channels} cannot be divisible by groups {groups}"
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = _pair(stride)
        self.padding = _pair(padding)
        self.dilation = _pair(dilation)
        self.groups = groups
        self.deformable_groups = deformable_groups
        self.transposed = False   # (compatibility with nn.Conv2d, as in the reference)
        self.output_padding = _single(0)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // self.groups, *self.kernel_size))
        self.reset_parameters()

    def reset_parameters(self):
        n = self.in_channels
        for k in self.kernel_size:
            n *= k
        stdv = 1. / math.sqrt(n)
        self.weight.data.uniform_(-stdv, stdv)

    def forward(self, x, offset):
        # an input smaller than the kernel is padded at the bottom / right, and the output cropped (deform_conv.py:239-255)
        input_pad = x.size(2) < self.kernel_size[0] or x.size(3) < self.kernel_size[1]
        if input_pad:
            pad_h = max(self.kernel_size[0] - x.size(2), 0)
            pad_w = max(self.kernel_size[1] - x.size(3), 0)
            x = F.pad(x, (0, pad_w, 0, pad_h), "constant", 0).contiguous()
            offset = F.pad(offset, (0, pad_w, 0, pad_h), "constant", 0).contiguous()
        out = _deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups, self.deformable_groups, self.fused_relu)
        if input_pad:
            out = out[:, :, :out.size(2) - pad_h, :out.size(3) - pad_w].contiguous()
        return out
