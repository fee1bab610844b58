"""The contracts of tests/autograd_contract.py can fail (no GPU, no native library).  A toy autograd.Function around stock F.conv2d and a
toy batch norm with a hand-written backward, built the way the product's layers are (weight image from a cache, dy normalised by hand,
epilogue statistics handed to the norm as an attribute on the tensor), pass every contract; each seeded defect is rejected by the contract
that exists for it, and the test asserts which one did."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import autograd_contract as AC

DEFECTS = {   # defect -> the contract that must reject it
    "dy_storage_order": "b",
    "mask_changes_forward": "a",
    "frozen_gets_grad": "a",
    "saved_mutated": "c",
    "last_call_state": "d",
    "stale_image": "f",
    "unstamped_tag": "h",
}
STATS = {"fwd_folded": 0}
_LAST = {}
_IMAGES = {}   # id(weight) -> (weight, version, image)


def _image(w, defect):
    ent = _IMAGES.get(id(w))
    if ent is not None and ent[0] is w and (defect == "stale_image" or ent[1] == w._version):
        return ent[2]
    img = w.detach().clone()
    _IMAGES[id(w)] = (w, w._version, img)
    return img


class _ToyConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, defect, emit):
        img = _image(weight, defect)
        y = F.conv2d(x, img, None if bias is None else bias.detach(), padding=1)
        if defect == "mask_changes_forward" and not ctx.needs_input_grad[0]:
            y = y.to(torch.bfloat16).float()
        ctx.save_for_backward(x, img)
        ctx.defect, ctx.weight_p, ctx.has_bias = defect, weight, bias is not None
        _LAST["x"] = x
        if emit:
            partial = torch.stack([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))])
            ctx.mark_non_differentiable(partial)
            return y, partial
        return y

    @staticmethod
    def backward(ctx, dy, *_unused):
        x, img = ctx.saved_tensors
        defect = ctx.defect
        if defect == "dy_storage_order":   # "it is dense in y's layout": reads the allocation as it lies
            n, c, h, w = dy.shape
            dy = dy.as_strided(dy.shape, (c * h * w, h * w, w, 1), dy.storage_offset())
        else:
            dy = dy.contiguous()
        if defect == "last_call_state":
            x = _LAST["x"]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.nn.grad.conv2d_input(x.shape, img, dy, padding=1)
        if ctx.needs_input_grad[1]:
            dw = torch.nn.grad.conv2d_weight(x, img.shape, dy, padding=1)
        elif defect == "frozen_gets_grad":
            ctx.weight_p.grad = torch.nn.grad.conv2d_weight(x, img.shape, dy, padding=1)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum((0, 2, 3))
        if defect == "saved_mutated":
            x.data.mul_(1.5)
        return dx, dw, db, None, None


class ToyConv(nn.Conv2d):
    defect = None
    emit_bn_stats = False

    def forward(self, x):
        if self.emit_bn_stats and self.training and torch.is_grad_enabled():
            y, partial = _ToyConvFn.apply(x, self.weight, self.bias, self.defect, True)
            y._toy_partial = (partial, y._version)
            return y
        return _ToyConvFn.apply(x, self.weight, self.bias, self.defect, False)


class _ToyNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, module, partial):
        n = x.numel() // x.shape[1]
        if partial is not None:
            STATS["fwd_folded"] += 1
            s1, s2 = partial[0], partial[1]
        else:
            s1, s2 = x.sum((0, 2, 3)), (x * x).sum((0, 2, 3))
        mean = s1 / n
        var = (s2 / n - mean * mean).clamp_min(0)
        invstd = torch.rsqrt(var + module.eps)
        with torch.no_grad():
            module.running_mean.mul_(1 - module.momentum).add_(module.momentum * mean)
            module.running_var.mul_(1 - module.momentum).add_(module.momentum * var * n / (n - 1))
        xh = (x - mean[None, :, None, None]) * invstd[None, :, None, None]
        ctx.save_for_backward(xh, gamma, invstd)
        return xh * gamma.detach()[None, :, None, None] + beta.detach()[None, :, None, None]

    @staticmethod
    def backward(ctx, dy):
        xh, gamma, invstd = ctx.saved_tensors
        n = xh.numel() // xh.shape[1]
        dgamma, dbeta = (dy * xh).sum((0, 2, 3)), dy.sum((0, 2, 3))
        g = dy * gamma.detach()[None, :, None, None]
        dx = (g - g.mean((0, 2, 3), keepdim=True) - xh * (g * xh).mean((0, 2, 3), keepdim=True)) * invstd[None, :, None, None]
        return dx, dgamma, dbeta, None, None


class ToyNorm(nn.BatchNorm2d):
    defect = None

    def forward(self, x):
        tag = getattr(x, "_toy_partial", None)
        partial = None
        if tag is not None and (self.defect == "unstamped_tag" or tag[1] == x._version):
            partial = tag[0]
        return _ToyNormFn.apply(x, self.weight, self.bias, self, partial)


def conv_case(defect, bias=True):
    def build(device):
        torch.manual_seed(5)
        m = ToyConv(4, 6, 3, padding=1, bias=bias).to(device)
        m.defect = defect
        return m

    def inputs(seed, device):
        g = torch.Generator().manual_seed(seed)
        return {"x": torch.randn(2, 4, 5, 7, generator=g).to(device)}

    def params(m):
        return {"weight": m.weight, **({"bias": m.bias} if bias else {})}

    def ref(ops):
        return F.conv2d(ops["x"], ops["weight"], ops.get("bias"), padding=1)
    # fp32 sums of at most 36 + 1 products (forward, dx) and 70 (dw, db) against float64: <= 70 * 2^-24 * sum|terms|, far inside 1e-4 of max
    tol = {k: 1e-4 for k in ("y", "x", "weight", "bias")}
    return AC.Case(f"toy_conv[{defect}]", build, inputs, lambda m, i: m(i["x"]), params, ref, tol, linear=True)


def pair_case(defect):
    def build(device):
        torch.manual_seed(6)
        conv, norm = ToyConv(4, 6, 3, padding=1).to(device), ToyNorm(6).to(device)
        conv.emit_bn_stats = True
        norm.defect = defect
        with torch.no_grad():
            norm.weight.uniform_(0.5, 1.5); norm.bias.uniform_(-0.5, 0.5)
        return conv, norm

    def norm_ref(z, gamma, beta):
        return F.batch_norm(z, None, None, gamma, beta, True, 0.0, 1e-5)

    def running_ref(z, before):
        n = z.numel() // z.shape[1]
        return {"running_mean": 0.9 * before["running_mean"] + 0.1 * z.mean((0, 2, 3)),
                "running_var": 0.9 * before["running_var"] + 0.1 * z.var((0, 2, 3), unbiased=False) * n / (n - 1)}
    tol = {"y": 1e-4, "z": 1e-4, "gamma": 1e-4, "beta": 1e-4, "running": 1e-4}
    return AC.PairCase(f"toy_conv_norm[{defect}]", build, lambda s, d: torch.randn(2, 4, 5, 7, generator=torch.Generator().manual_seed(s)).to(d),
                       lambda conv, x: conv(x), lambda norm, z: norm(z), lambda norm: {"gamma": norm.weight, "beta": norm.bias}, norm_ref,
                       lambda norm: {"running_mean": norm.running_mean, "running_var": norm.running_var}, running_ref,
                       lambda: STATS["fwd_folded"], tol)


def battery(defect):
    """-> {contract: ContractError or None} over every contract"""
    case, pair = conv_case(defect), pair_case(defect)
    runs = {
        "a": lambda: AC.contract_masks(case, "cpu"),
        "b": lambda: AC.contract_grad_forms(case, "cpu"),
        "c": lambda: AC.contract_replay(case, "cpu"),
        "d": lambda: (AC.contract_interleave(case, "cpu"), AC.contract_accumulate(case, "cpu")),
        "e": lambda: AC.contract_grad_mode(case, "cpu"),
        "f": lambda: AC.contract_param_update(case, "cpu"),
        "g": lambda: AC.contract_fanout(case, "cpu"),
        "h": lambda: [AC.contract_stale_tags(pair, "cpu", op) for op in AC.INPLACE_OPS],
    }
    out = {}
    for k, fn in runs.items():
        _IMAGES.clear()
        try:
            fn()
            out[k] = None
        except AC.ContractError as e:
            out[k] = e
    return out


def test_the_clean_function_passes_every_contract():
    res = battery(None)
    assert all(v is None for v in res.values()), {k: str(v) for k, v in res.items() if v is not None}
    case = conv_case(None, bias=False)
    AC.contract_masks(case, "cpu")
    AC.contract_param_update(case, "cpu")


@pytest.mark.parametrize("defect,contract", sorted(DEFECTS.items()))
def test_each_defect_is_rejected_by_its_contract(defect, contract):
    res = battery(defect)
    err = res[contract]
    assert err is not None, f"{defect}: contract ({contract}) accepted it; rejected by {[k for k, v in res.items() if v is not None]}"
    assert err.contract == contract and err.case.endswith(f"[{defect}]")
    print(f"{defect}: rejected by {sorted(k for k, v in res.items() if v is not None)}; ({contract}) said: {err}")


def test_the_messages_name_case_contract_leaf_and_elements():
    err = battery("stale_image")["f"]
    text = str(err)
    assert "toy_conv[stale_image]" in text and "contract (f)" in text and "leaf y" in text and "differ, first (0, 0, 0, 0):" in text


def test_grad_forms_hold_the_same_values_in_the_layouts_they_name():
    G = torch.randn(2, 16, 3, 5).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    forms = dict(AC.grad_forms(G))
    assert forms["other_memory_format"].is_contiguous() and not forms["other_memory_format"].is_contiguous(memory_format=torch.channels_last)
    a, u = forms["slice_aligned"], forms["slice_unaligned"]
    assert a.stride(1) == 1 and a.stride(3) % 8 == 0 and a.stride(3) > 16 and (a.storage_offset() * 2) % 16 == 0
    assert u.stride(1) == 1 and u.storage_offset() % 8 != 0
    assert forms["spatial_transposed"].stride(2) < forms["spatial_transposed"].stride(3)
    M = torch.randn(11, 32)
    f2 = dict(AC.grad_forms(M))
    assert f2["row_strided"].stride(0) == 64 and f2["column_slice"].stride(0) == 56 and f2["column_slice"].storage_offset() == 8
