"""The autograd contract (tests/autograd_contract.py) of the layers with hand-written backwards: what the Python between autograd and the
kernels does when the trainable set, the layout of the upstream gradient, the call order or the parameters change.  The kernel parity
suites hold all of these constant; here the kernels are taken as given and everything else moves.

Shapes are the smallest that still take the HIP path.  Tolerances are those of each layer's existing float64 test (named per case);
layers without one take 8e-3 (bf16-stored) / 2e-3 (fp32) of max|ref|, derived in the header of tests/test_s16_gpu.py.

EXEMPT lists the only gradients that are not held to bit equality: they are summed with float atomics, so their bits depend on the
order in which workgroups arrive.  They are held to their float64 tolerance wherever a bit equality is asked."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import autograd_contract as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (case name pattern, leaf) -> file:line of the float atomic that sums it
EXEMPT = {
    ("conv3x3_128_64_s2_8x6", "weight"): "sparse2dense_amd/dense2d.py:403 (aten.convolution_backward: MIOpen's bf16 weight gradient, summed outside this "
                                         "repository; two runs on the same operands differ in single bf16 elements)",
    ("conv3x3_128_64_s2_9x7", "weight"): "sparse2dense_amd/dense2d.py:403 (the same call)",
    ("deform_conv_64_64_dg4", "x"): "sparse2dense_amd/csrc/deform_conv.hip:357 (unsafeAtomicAdd into the fp32 image of dX; "
                                    "tests/test_deform_conv_gpu.py::test_outputs_without_atomics_are_bit_identical_from_run_to_run)",
}


def test_the_exemption_table_is_the_whole_list():
    assert {(c.name, leaf) for c in cases().values() for leaf in c.inexact} == set(EXEMPT)



def _D():
    from sparse2dense_amd import dense2d
    return dense2d


def _side():
    from sparse2dense_amd import side
    return side


def _sync():
    _side().join()


@contextlib.contextmanager
def side_all():
    side = _side()
    prev = side.MODE
    side.enable("all")
    try:
        yield
    finally:
        side.join()
        side.MODE = prev


def autocast():
    return torch.autocast("cuda", torch.bfloat16)


def rb(t):
    return t.to(torch.bfloat16).float()


def nhwc16(t):
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ----------------------------------------------------------------------------------------------------------------------------------
# dense 2D: bf16 channels_last inputs under bf16 autocast, N = 2
def conv_case(name, make, hw, ref, tol, cin, bias=True, repack=False, uses_side=True, round_w=True, inexact=()):
    def build(device):
        torch.manual_seed(17)
        m = make().to(device).train()
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(rb(p) if round_w else p)
        return m

    def inputs(seed, device):
        return {"x": nhwc16(_randn((2, cin) + hw, seed).to(device))}

    def params(m):
        return {"weight": m.weight, **({"bias": m.bias} if m.bias is not None else {})}
    case = AC.Case(name, build, inputs, lambda m, i: m(i["x"]), params, ref, tol, context=autocast, linear=True, sync=_sync, inexact=inexact)
    case.repack, case.uses_side = repack, uses_side
    return case


def _conv_ref(stride=1, padding=0, groups=1):
    return lambda o: F.conv2d(o["x"], o["weight"], o.get("bias"), stride=stride, padding=padding, groups=groups)


def _convt_ref(stride, padding=0):
    return lambda o: F.conv_transpose2d(o["x"], o["weight"], o.get("bias"), stride=stride, padding=padding)


def dense_conv_cases():
    D = _D()
    T3 = {"y": 6e-3, "x": 6e-3, "weight": 1e-3, "bias": 1e-3}      # test_forward_and_dgrad, test_conv3x3_wgrad_matches_float64, ..._at_bev_size
    TS2 = {"y": 6e-3, "x": 6e-3, "weight": 2e-3, "bias": 2e-3}     # tests/test_conv_s2_gpu.py
    TS2F = {"y": 6e-3, "x": 1e-2, "weight": 1e-2, "bias": 2e-3}    # test_stride2_forward_and_module_backward, test_module_autograd_matches_stock_conv (MIOpen bf16)
    T1 = {"y": 6e-3, "x": 6e-3, "weight": 2e-3, "bias": 2e-3}      # test_conv1x1_..., test_conv2x2_stride2_..., test_conv_transpose_2x2_...
    TSM = {"y": 1e-5, "x": 4e-3, "weight": 1e-5, "bias": 1e-5}     # test_small_cout_conv3x3_forward_backward_vs_cpu_float64
    TDW = {"y": 6e-3, "x": 6e-3, "weight": 2e-3, "bias": 2e-3}     # test_depthwise7_forward_backward_vs_cpu_float64
    return [
        conv_case("conv3x3_64_64_p1_bias", lambda: D.Conv3x3(64, 64, 3, 1, 1), (6, 5), _conv_ref(1, 1), T3, 64, repack=True),
        conv_case("conv3x3_64_64_p1_nobias", lambda: D.Conv3x3(64, 64, 3, 1, 1, bias=False), (6, 5), _conv_ref(1, 1), T3, 64, repack=True),
        conv_case("conv3x3_64_128_p0", lambda: D.Conv3x3(64, 128, 3, 1, 0), (6, 5), _conv_ref(1, 0), T3, 64, repack=True),
        # stride 2: the data-gradient kernel needs cout >= 128 (convup_supported), so 64 -> 128 on 8x6 takes `_s2_backward_ok`'s kernels and
        # 128 -> 64 takes MIOpen at both sizes (8x6 by its channels, 9x7 by its odd size)
        conv_case("conv3x3_64_128_s2_8x6", lambda: D.Conv3x3(64, 128, 3, 2, 1), (8, 6), _conv_ref(2, 1), TS2, 64, repack=True),
        conv_case("conv3x3_128_64_s2_8x6", lambda: D.Conv3x3(128, 64, 3, 2, 1), (8, 6), _conv_ref(2, 1), TS2F, 128, repack=True, uses_side=False,
                  inexact=("weight",)),
        conv_case("conv3x3_128_64_s2_9x7", lambda: D.Conv3x3(128, 64, 3, 2, 1), (9, 7), _conv_ref(2, 1), TS2F, 128, repack=True, uses_side=False,
                  inexact=("weight",)),
        conv_case("conv1x1_64_128_bias", lambda: D.Conv1x1(64, 128, 1), (6, 5), _conv_ref(), T1, 64, repack=True),
        conv_case("conv1x1_64_128_nobias", lambda: D.Conv1x1(64, 128, 1, bias=False), (6, 5), _conv_ref(), T1, 64, repack=True),
        conv_case("smallconv3x3_64_3", lambda: D.SmallConv3x3(64, 3, 3, padding=1), (6, 5), _conv_ref(1, 1), TSM, 64, round_w=False),
        conv_case("smallconv3x3_8_1", lambda: D.SmallConv3x3(8, 1, 3, padding=1), (6, 5), _conv_ref(1, 1), TSM, 8, round_w=False),
        conv_case("conv2x2s2_64_64", lambda: D.Conv2x2S2(64, 64, 2, 2), (8, 6), _conv_ref(2, 0), T1, 64, repack=True),
        conv_case("convt2x2s2_64_64", lambda: D.ConvT2x2S2(64, 64, 2, 2), (6, 5), _convt_ref(2), T1, 64, repack=True),
        conv_case("convt4x4s2_128_64", lambda: D.ConvT4x4S2(128, 64, 4, 2, 1), (6, 5), _convt_ref(2, 1), TS2, 128, repack=True),
        conv_case("depthwise7_8", lambda: D.DepthwiseConv7(8, 8, 7, padding=3, groups=8), (9, 5), _conv_ref(1, 3, 8), TDW, 8, round_w=False),
        conv_case("depthwise7_264", lambda: D.DepthwiseConv7(264, 264, 7, padding=3, groups=264), (9, 5), _conv_ref(1, 3, 264), TDW, 264, round_w=False),
    ]


def _act(y, relu):
    return F.gelu(y) if int(relu) == 2 else (torch.relu(y) if relu else y)


TBN = {"y": 1e-2, "x": 1.5e-2, "gamma": 2e-3, "beta": 2e-3}   # test_fast_batchnorm2d_training
TBN_EVAL = dict(TBN, x=1e-2)                                  # test_fast_batchnorm2d_eval_and_fallbacks: y and dx 1e-2


def bn2d_case(c, relu, training, frozen_affine=False):
    D = _D()

    def build(device):
        torch.manual_seed(23)
        m = D.FastBatchNorm2d(c, eps=1e-3, momentum=0.1, fused_relu=relu).to(device)
        with torch.no_grad():
            m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5); m.running_mean.uniform_(-0.5, 0.5); m.running_var.uniform_(0.5, 2.0)
        return m.train(training)

    def inputs(seed, device):
        return {"x": nhwc16((_randn((2, c, 6, 5), seed) * 1.5 + 0.3).to(device))}

    def ref(o):
        if training:
            y = F.batch_norm(o["x"], None, None, o["gamma"], o["beta"], True, 0.0, 1e-3)
        else:
            y = F.batch_norm(o["x"], o["running_mean"], o["running_var"], o["gamma"], o["beta"], False, 0.0, 1e-3)
        return _act(y, relu)

    def call(m, i):
        i["running_mean"], i["running_var"] = m.running_mean.clone(), m.running_var.clone()   # (what an eval forward reads)
        if frozen_affine:   # the distillation teacher: the affine is no leaf, every contract runs on _BNRowFn's [mean, invstd, scale, shift] cache
            m.weight.requires_grad_(False); m.bias.requires_grad_(False)
            i["gamma"], i["beta"] = m.weight.detach().clone(), m.bias.detach().clone()
            y = m(i["x"])
            assert getattr(m, "_s2d_eval_fin", None) is not None, "control: a frozen eval-mode affine takes the cache"
            return y
        return m(i["x"])
    name = f"bn2d_c{c}_relu{int(relu)}_{'train' if training else 'eval'}" + ("_frozen" if frozen_affine else "")
    params = (lambda m: {}) if frozen_affine else (lambda m: {"gamma": m.weight, "beta": m.bias})
    case = AC.Case(name, build, inputs, call, params, ref, TBN if training else TBN_EVAL, has_stats=True, sync=_sync)
    case.repack, case.uses_side = False, False
    return case


def bn2d_cases():
    out = []
    for c in (8, 64):
        for relu in (0, 1, 2):
            out.append(bn2d_case(c, relu, True))
            out.append(bn2d_case(c, relu, False))
        out.append(bn2d_case(c, 1, False, frozen_affine=True))
    return out


def ln_case(nhwc):
    D = _D()
    TLN = {"y": 6e-3, "x": 6e-3, "weight": 1e-4, "bias": 1e-4}   # test_wide_layernorm_bf16_kernels_vs_float64

    def build(device):
        torch.manual_seed(29)
        m = D.WideLayerNorm([64, 32, 32], eps=1e-6).to(device)
        with torch.no_grad():
            m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5)
        return m

    def inputs(seed, device):
        x = (_randn((2, 64, 32, 32), seed) * 1.5 + 0.3).to(device).to(torch.bfloat16)
        return {"x": x.contiguous(memory_format=torch.channels_last) if nhwc else x.contiguous()}
    case = AC.Case(f"widelayernorm_{'nhwc' if nhwc else 'nchw'}", build, inputs, lambda m, i: m(i["x"]), lambda m: {"weight": m.weight, "bias": m.bias},
                   lambda o: F.layer_norm(o["x"], [64, 32, 32], o["weight"], o["bias"], 1e-6), TLN, sync=_sync)
    case.repack, case.uses_side = False, False
    return case


def resample_case(up):
    from sparse2dense_amd import pillars as P
    T = {"y": 8e-3, "x": 8e-3}   # bf16-stored (both are exact selections / sums of at most four bf16 values)

    def build(device):
        return P._UpsampleKeepDtype(scale_factor=2, mode="nearest") if up else P.MaxPool2x2(2, 2)

    def inputs(seed, device):
        return {"x": nhwc16(_randn((2, 8, 6, 4), seed).to(device))}
    ref = (lambda o: F.interpolate(o["x"], scale_factor=2, mode="nearest")) if up else (lambda o: F.max_pool2d(o["x"], 2, 2))
    case = AC.Case("upsample2x_c8" if up else "maxpool2x2_c8", build, inputs, lambda m, i: m(i["x"]), lambda m: {}, ref, T, context=autocast, sync=_sync)
    case.repack, case.uses_side = False, False
    return case


def row_linear_case():
    from sparse2dense_amd import pillars as P
    T = {"y": 1e-5, "x": 1e-5, "weight": 1e-5}   # tests/test_pillars.py::test_row_linear_weight_gradient_kernel_matches_float64: 1e-5 of max

    def build(device):
        torch.manual_seed(31)
        return torch.nn.Linear(10, 32, bias=False).to(device)

    def inputs(seed, device):
        return {"x": _randn((111, 10), seed).to(device)}
    case = AC.Case("row_linear_111_10_32", build, inputs, lambda m, i: P._row_linear(i["x"].view(111, 1, 10), m).view(111, 32), lambda m: {"weight": m.weight},
                   lambda o: o["x"] @ o["weight"].t(), T, linear=True, sync=_sync)
    case.repack, case.uses_side = False, False
    return case



def bn2d_out_slice_case(c):
    """two training-mode batch norms writing channel slices of one buffer (`out=`), joined by _CatSlicesFn: the RPN's up-sampling branches"""
    D = _D()

    def build(device):
        torch.manual_seed(43)
        m = torch.nn.ModuleList([D.FastBatchNorm2d(c, eps=1e-3, momentum=0.1, fused_relu=True) for _ in range(2)]).to(device).train()
        with torch.no_grad():
            for b in m:
                b.weight.uniform_(0.5, 1.5); b.bias.uniform_(-0.5, 0.5)
        return m

    def inputs(seed, device):
        return {"x": nhwc16((_randn((2, c, 6, 5), seed) * 1.5 + 0.3).to(device)), "x2": nhwc16((_randn((2, c, 6, 5), seed + 50) - 0.2).to(device))}

    def call(m, i):
        buf = torch.empty((2, 2 * c, 6, 5), dtype=torch.bfloat16, device=i["x"].device).contiguous(memory_format=torch.channels_last)
        ya, yb = m[0](i["x"], out=buf[:, :c]), m[1](i["x2"], out=buf[:, c:])
        i["gamma2"], i["beta2"] = m[1].weight.detach().clone(), m[1].bias.detach().clone()
        return D._CatSlicesFn.apply(buf, ya, yb)

    def ref(o):
        return torch.cat([torch.relu(F.batch_norm(o["x"], None, None, o["gamma"], o["beta"], True, 0.0, 1e-3)),
                          torch.relu(F.batch_norm(o["x2"], None, None, o["gamma2"], o["beta2"], True, 0.0, 1e-3))], 1)
    case = AC.Case(f"bn2d_c{c}_out_slice_cat", build, inputs, call, lambda m: {"gamma": m[0].weight, "beta": m[0].bias}, ref, TBN, has_stats=True, sync=_sync)
    case.repack, case.uses_side = False, False
    return case


# ----------------------------------------------------------------------------------------------------------------------------------
# sparse: a two-frame random grid (9, 12, 11) at occupancy 0.4
GRID = (9, 12, 11)


def _sparse_indices(device):
    g = torch.Generator().manual_seed(3)
    occ = torch.rand((2,) + GRID, generator=g) < 0.4
    return occ.nonzero().int().to(device)


def _scatter(vol, feat, idx):
    b, c = vol.shape[:2]
    flat = vol.permute(0, 2, 3, 4, 1).reshape(-1, c)
    d, h, w = vol.shape[2:]
    lin = ((idx[:, 0] * d + idx[:, 1]) * h + idx[:, 2]) * w + idx[:, 3]
    flat = flat.index_add(0, lin, feat)   # (sites are unique: an add is a write, and it is differentiable)
    return flat.reshape(b, d, h, w, c).permute(0, 4, 1, 2, 3)


def sparse_conv_case(name, subm, cin, cout, k, stride, pad, mode, sorted_rows=None):
    from sparse2dense_amd import spconv as S
    from sparse2dense_amd import hip_ops as H
    s16 = mode == "s16"
    # header of tests/test_s16_gpu.py: 8e-3 of max for bf16-stored results, 2e-3 for fp32 ones
    tol = {"y": 8e-3, "x": 8e-3, "weight": 2e-3, "bias": 2e-3} if s16 else {k_: 2e-3 for k_ in ("y", "x", "weight", "bias")}

    def build(device):
        torch.manual_seed(47)
        m = (S.SubMConv3d(cin, cout, k, padding=pad, indice_key="k") if subm else S.SparseConv3d(cin, cout, k, stride, pad)).to(device).train()
        with torch.no_grad():
            m.weight.copy_(rb(m.weight))
        return m

    def inputs(seed, device):
        idx = _sparse_indices(device)
        x = _randn((idx.shape[0], cin), seed).to(device)
        return {"x": x.to(torch.bfloat16) if s16 else rb(x), "idx": idx}

    @contextlib.contextmanager
    def scope():   # both globals are read again at backward time (spconv._SparseConvFn.backward -> _s16 -> hip_ops.spconv_s16_sorted_ok)
        prev, was = H.SPARSE_COMPUTE_DTYPE, None
        H.set_sparse_compute_dtype(mode)
        if sorted_rows is not None:
            was = H.set_sorted_rows(sorted_rows)
        try:
            yield
        finally:
            H.set_sparse_compute_dtype(prev)
            if was is not None:
                H.set_sorted_rows(was)

    def call(m, i):
        out = m(S.SparseConvTensor(i["x"], i["idx"], GRID, 2))
        i["out_idx"], i["out_shape"] = out.indices, torch.tensor(out.spatial_shape)
        return out.features

    def ref(o):
        kk = (k,) * 3 if isinstance(k, int) else tuple(k)
        st = (stride,) * 3 if isinstance(stride, int) else tuple(stride)
        pd = (pad,) * 3 if isinstance(pad, int) else tuple(pad)
        vol = _scatter(o["x"].new_zeros((2, cin) + GRID), o["x"], o["idx"].long())
        w = o["weight"].permute(4, 3, 0, 1, 2)   # [kz, ky, kx, cin, cout] -> [cout, cin, kz, ky, kx]
        y = F.conv3d(vol, w, o.get("bias"), stride=(1, 1, 1) if subm else st, padding=pd)
        oi = o["out_idx"].long()
        assert tuple(y.shape[2:]) == tuple(int(v) for v in o["out_shape"].tolist())
        return y[oi[:, 0], :, oi[:, 1], oi[:, 2], oi[:, 3]]
    case = AC.Case(name, build, inputs, call, lambda m: {"weight": m.weight, **({"bias": m.bias} if m.bias is not None else {})}, ref, tol,
                   scope=scope, linear=True, sync=_sync)
    case.repack, case.uses_side, case.sorted_rows = True, s16, sorted_rows   # (the fp32 path keeps its weight gradient on the chain)
    return case


def sparse_cases():
    out = []
    for mode in ("f32", "s16"):
        out += [sparse_conv_case(f"subm_16_16_{mode}", True, 16, 16, 3, 1, 1, mode),
                sparse_conv_case(f"subm_64_128_{mode}", True, 64, 128, 3, 1, 1, mode)]
        # sorted rows exist on the bf16-storage path only: one fp32 case, the s16 one with the form on and off
        out += ([sparse_conv_case("subm_128_128_f32", True, 128, 128, 3, 1, 1, mode)] if mode == "f32" else
                [sparse_conv_case("subm_128_128_sorted_s16", True, 128, 128, 3, 1, 1, mode, sorted_rows=True),
                 sparse_conv_case("subm_128_128_unsorted_s16", True, 128, 128, 3, 1, 1, mode, sorted_rows=False)])
        out += [
                sparse_conv_case(f"spconv_k3s2p1_32_64_{mode}", False, 32, 64, 3, 2, 1, mode),
                sparse_conv_case(f"spconv_k311s211_128_128_{mode}", False, 128, 128, (3, 1, 1), (2, 1, 1), 0, mode)]
    return out


def feature_bn_case(bf16, training):
    from sparse2dense_amd import spconv as S
    c = 32
    # bf16: the row kernels of FastBatchNorm2d (test_fast_batchnorm2d_training); fp32: 2e-3 of max (header of tests/test_s16_gpu.py)
    tol = (dict(TBN, residual=TBN["x"]) if training else dict(TBN_EVAL, residual=TBN_EVAL["x"])) if bf16 else {k: 2e-3 for k in ("y", "x", "residual", "gamma", "beta")}

    def build(device):
        torch.manual_seed(53)
        m = S.FeatureBatchNorm1d(c, eps=1e-3, momentum=0.1).to(device)
        with torch.no_grad():
            m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5); m.running_mean.uniform_(-0.5, 0.5); m.running_var.uniform_(0.5, 2.0)
        return m.train(training)

    def inputs(seed, device):
        x, r = (_randn((333, c), seed) * 1.5 + 0.3).to(device), _randn((333, c), seed + 70).to(device)
        return {"x": x.to(torch.bfloat16), "residual": r.to(torch.bfloat16)} if bf16 else {"x": x, "residual": r}

    def call(m, i):
        i["running_mean"], i["running_var"] = m.running_mean.clone(), m.running_var.clone()
        return m(i["x"], residual=i["residual"], relu=True)

    def ref(o):
        y = F.batch_norm(o["x"], None if training else o["running_mean"], None if training else o["running_var"], o["gamma"], o["beta"], training, 0.0, 1e-3)
        return torch.relu(y + o["residual"])
    case = AC.Case(f"feature_bn1d_{'bf16' if bf16 else 'fp32'}_res_relu_{'train' if training else 'eval'}", build, inputs, call,
                   lambda m: {"gamma": m.weight, "beta": m.bias}, ref, tol, leaves=("x", "residual"), has_stats=True, sync=_sync)
    case.repack, case.uses_side = False, False
    return case


def densify_case(bev):
    from sparse2dense_amd import spconv as S
    c = 16
    tol = {"y": 8e-3, "x": 8e-3} if bev else {"y": 2e-3, "x": 2e-3}   # (both are copies: any error at all is a defect)

    def inputs(seed, device):
        idx = _sparse_indices(device)
        x = _randn((idx.shape[0], c), seed).to(device)
        return {"x": x.to(torch.bfloat16) if bev else x, "idx": idx}

    def call(m, i):
        t = S.SparseConvTensor(i["x"], i["idx"], GRID, 2)
        return t.dense_bev(nhwc_bf16=True) if bev else t.dense()

    def ref(o):
        vol = _scatter(o["x"].new_zeros((2, c) + GRID), o["x"], o["idx"].long())
        return vol.reshape(2, c * GRID[0], GRID[1], GRID[2]) if bev else vol
    case = AC.Case("dense_bev_nhwc_bf16" if bev else "sparse_dense", lambda device: torch.nn.Identity(), inputs, call, lambda m: {}, ref, tol, sync=_sync)
    case.repack, case.uses_side = False, False
    return case


# ----------------------------------------------------------------------------------------------------------------------------------
# dense 3D: fp32 NCDHW, no autocast
def _bf16_grad(y, seed):
    return AC.default_grad(y, seed).to(torch.bfloat16).to(y.dtype)


def conv3d_case(name, make, cin, pos, ref, tol, bf16=False):
    def build(device):
        torch.manual_seed(59)
        m = make().to(device).train()
        m.bf16_compute = bf16
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(rb(p))
        return m
    case = AC.Case(name, build, lambda s, d: {"x": rb(_randn((2, cin) + pos, s)).to(d)}, lambda m, i: m(i["x"]),
                   lambda m: {"weight": m.weight, **({"bias": m.bias} if m.bias is not None else {})}, ref, tol, linear=True, sync=_sync,
                   grad_like=_bf16_grad)
    case.repack, case.uses_side = True, True
    return case


def dense3d_cases():
    from sparse2dense_amd import dense3d as D3
    T32 = {k: 1e-4 for k in ("y", "x", "weight", "bias")}    # tests/test_dense3d_gpu.py: 1e-4 of max on outputs and gradients
    T16 = T32   # tests/test_dense3d_gpu.py::test_convtranspose3d_bf16_mfma: 1e-4 of max over bf16-rounded operands and upstream gradient
    pw = lambda o: F.conv3d(o["x"], o["weight"], o.get("bias"))
    ct = lambda o: F.conv_transpose3d(o["x"], o["weight"], o.get("bias"), stride=2, padding=1)
    out = [conv3d_case("pointwise3d_32_3", lambda: D3.PointwiseConv3d(32, 3, 1), 32, (3, 6, 8), pw, T32),
           conv3d_case("pointwise3d_128_32", lambda: D3.PointwiseConv3d(128, 32, 1), 128, (3, 6, 8), pw, T32)]
    for bf in (False, True):
        t = T16 if bf else T32
        out += [conv3d_case(f"convt3d_16_3_{'bf16' if bf else 'fp32'}", lambda: D3.ConvTranspose3dK4S2(16, 3, 4, 2, 1), 16, (2, 3, 4), ct, t, bf),
                conv3d_case(f"convt3d_32_32_{'bf16' if bf else 'fp32'}", lambda: D3.ConvTranspose3dK4S2(32, 32, 4, 2, 1), 32, (2, 3, 4), ct, t, bf)]
    TB3 = {"y": 1e-4, "x": 1e-3, "gamma": 1e-3, "beta": 1e-3}   # test_dense3d_gpu.py batch-norm test: outputs 1e-4, gradients 1e-3 of max
    for c in (3, 32):
        for training in (True, False):
            def build(device, c=c, training=training):
                torch.manual_seed(61)
                m = D3.FastBatchNorm3d(c, eps=1e-5, momentum=0.1, fused_relu=True).to(device)
                with torch.no_grad():
                    m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.5, 0.5); m.running_mean.uniform_(-0.5, 0.5); m.running_var.uniform_(0.5, 2.0)
                return m.train(training)

            def call(m, i):
                i["running_mean"], i["running_var"] = m.running_mean.clone(), m.running_var.clone()
                return m(i["x"])

            def ref(o, training=training):
                return torch.relu(F.batch_norm(o["x"], None if training else o["running_mean"], None if training else o["running_var"],
                                               o["gamma"], o["beta"], training, 0.0, 1e-5))
            case = AC.Case(f"bn3d_c{c}_{'train' if training else 'eval'}", build,
                           lambda s, d, c=c: {"x": (_randn((2, c, 3, 6, 8), s) * 1.5 + 0.3).to(d)}, call,
                           lambda m: {"gamma": m.weight, "beta": m.bias}, ref, TB3, has_stats=True, sync=_sync)
            case.repack, case.uses_side = False, False
            out.append(case)
    return out



# ----------------------------------------------------------------------------------------------------------------------------------
def dcn_case():
    """dcn.DeformConv at (2, 64, 13, 11), 3x3, four deformable groups: the smallest shape tests/test_deform_conv_gpu.py runs on the kernels.
    Offsets on the 1/8 grid (exact in bf16 and fp32: no floor can fall differently in float64), reference dcn.deform_conv_composite in float64
    as in that file, 6e-3 of max for every tensor."""
    from sparse2dense_amd import dcn
    T = {k: 6e-3 for k in ("y", "x", "offset", "weight")}

    def build(device):
        torch.manual_seed(67)
        m = dcn.DeformConv(64, 64, 3, padding=1, deformable_groups=4).to(device)
        with torch.no_grad():
            m.weight.copy_(rb(m.weight))
        return m

    def inputs(seed, device):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(2, 64, 13, 11, generator=g)
        off = torch.randint(-40, 41, (2, 72, 13, 11), generator=g).float() / 8
        return {"x": nhwc16(x.to(device)), "offset": off.to(device).contiguous(memory_format=torch.channels_last)}
    case = AC.Case("deform_conv_64_64_dg4", build, inputs, lambda m, i: m(i["x"], i["offset"]), lambda m: {"weight": m.weight},
                   lambda o: dcn.deform_conv_composite(o["x"], o["offset"], o["weight"], 1, 1, 1, 1, 4), T, leaves=("x", "offset"),
                   context=autocast, sync=_sync, inexact=("x",))
    case.repack, case.uses_side = True, True
    return case


def _all_cases():
    return (dense_conv_cases() + bn2d_cases() + [bn2d_out_slice_case(8), bn2d_out_slice_case(64)]
            + [ln_case(False), ln_case(True), resample_case(False), resample_case(True), row_linear_case()]
            + sparse_cases() + [feature_bn_case(b, t) for b in (False, True) for t in (True, False)] + [densify_case(False), densify_case(True)]
            + dense3d_cases() + [dcn_case()])


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in _all_cases()}
    return _CASES


CONV_NAMES = ["conv3x3_64_64_p1_bias", "conv3x3_64_64_p1_nobias", "conv3x3_64_128_p0", "conv3x3_64_128_s2_8x6", "conv3x3_128_64_s2_8x6", "conv3x3_128_64_s2_9x7",
              "conv1x1_64_128_bias", "conv1x1_64_128_nobias", "smallconv3x3_64_3", "smallconv3x3_8_1", "conv2x2s2_64_64", "convt2x2s2_64_64",
              "convt4x4s2_128_64", "depthwise7_8", "depthwise7_264"]
BN_NAMES = [f"bn2d_c{c}_relu{r}_{m}" for c in (8, 64) for r in (0, 1, 2) for m in ("train", "eval")] + ["bn2d_c8_relu1_eval_frozen", "bn2d_c64_relu1_eval_frozen"]
OTHER_NAMES = ["bn2d_c8_out_slice_cat", "bn2d_c64_out_slice_cat", "widelayernorm_nchw", "widelayernorm_nhwc", "maxpool2x2_c8", "upsample2x_c8",
               "row_linear_111_10_32"]
SPARSE_CONV_NAMES = ["subm_128_128_f32", "subm_128_128_sorted_s16", "subm_128_128_unsorted_s16"] + [f"{n}_{m}" for m in ("f32", "s16") for n in ("subm_16_16", "subm_64_128",
                                                                 "spconv_k3s2p1_32_64", "spconv_k311s211_128_128")]
SPARSE_OTHER_NAMES = [f"feature_bn1d_{d}_res_relu_{t}" for d in ("fp32", "bf16") for t in ("train", "eval")] + ["sparse_dense", "dense_bev_nhwc_bf16"]
CONV3D_NAMES = ["pointwise3d_32_3", "pointwise3d_128_32", "convt3d_16_3_fp32", "convt3d_32_32_fp32", "convt3d_16_3_bf16", "convt3d_32_32_bf16"]
BN3D_NAMES = [f"bn3d_c{c}_{t}" for c in (3, 32) for t in ("train", "eval")]
LINEAR_NAMES = CONV_NAMES + ["row_linear_111_10_32"] + SPARSE_CONV_NAMES + CONV3D_NAMES
ALL_NAMES = CONV_NAMES + BN_NAMES + OTHER_NAMES + SPARSE_CONV_NAMES + SPARSE_OTHER_NAMES + CONV3D_NAMES + BN3D_NAMES + ["deform_conv_64_64_dg4"]


@pytest.fixture(scope="module", autouse=True)
def _record():
    """S2D_CONTRACT_RECORD=<path>: the per-case table of profiles/autograd_contract.txt, written when the module is done"""
    yield
    import os
    path = os.environ.get("S2D_CONTRACT_RECORD")
    if not path:
        return
    rows = {}
    for (case, contract), r in sorted(AC.RECORD.items()):
        row = rows.setdefault(case, {"c": [], "bit": 0, "tol": 0, "ratio": 0.0})
        row["c"].append(f"{contract}:{r['status']}")
        row["bit"], row["tol"], row["ratio"] = row["bit"] + r["bit"], row["tol"] + r["tol"], max(row["ratio"], r["max_ratio"])
    lines = [f"{'case':<40}{'bit-eq':>8}{'toler.':>8}{'worst err/bound':>17}  contracts"]
    lines += [f"{case:<40}{r['bit']:>8}{r['tol']:>8}{r['ratio']:>17.3f}  {' '.join(r['c'])}" for case, r in rows.items()]
    lines += ["", f"bit-equality comparisons made: {AC.TALLY['bit']}",
              f"toleranced comparisons made:   {AC.TALLY['tol']}, largest |error| / bound {AC.TALLY['max_ratio']:.3f}", "",
              "exempt from bit equality (float atomics; held to the float64 tolerance instead):"]
    lines += [f"  {c} d{leaf}: {why}" for (c, leaf), why in sorted(EXEMPT.items())]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


@pytest.fixture(autouse=True)
def _clean_globals():
    """every global a contract flips is restored, whatever the test did"""
    D, side = _D(), _side()
    from sparse2dense_amd import hip_ops as H
    saved = (side.MODE, D.BN_BWD_FOLD, D.ENABLED, H.SPARSE_COMPUTE_DTYPE)
    D.clear_pack_cache()
    try:
        yield
    finally:
        side.join()
        side.MODE, D.BN_BWD_FOLD, D.ENABLED = saved[:3]
        H.set_sparse_compute_dtype(saved[3])
        D.clear_pack_cache()


def test_the_case_table_is_the_one_named_here():
    assert sorted(cases()) == sorted(ALL_NAMES)


FUNCTIONS = [("conv3x3_", "_Conv3x3Fn"), ("conv1x1_", "_Conv1x1Fn"), ("smallconv3x3_", "_SmallConv3x3Fn"), ("conv2x2s2_", "_Conv2x2S2Fn"),
             ("convt2x2s2_", "_ConvT2x2S2Fn"), ("convt4x4s2_", "_ConvT4x4S2Fn"), ("depthwise7_", "_DwConv7Fn"), ("bn2d_", "_BNRowFn"),
             ("widelayernorm_", "_WideLNFn"), ("maxpool2x2_", "_Resample2x2Fn"), ("upsample2x_", "_Resample2x2Fn"), ("row_linear_", "_RowLinearFn"),
             ("subm_", "_SparseConvFn"), ("spconv_", "_SparseConvFn"), ("feature_bn1d_fp32_res_relu_train", "_BNTrainFn"),
             ("feature_bn1d_fp32_res_relu_eval", "_BNEvalFn"), ("feature_bn1d_bf16", "_BNRowFn"), ("sparse_dense", "_Densify"),
             ("dense_bev_", "_DensifyBev"), ("pointwise3d_", "_PwConvFn"), ("convt3d_", "_ConvT3dFn"), ("bn3d_", "_BNChannelMajorFn"),
             ("deform_conv_", "_DeformConvHipFn")]


@pytest.mark.parametrize("name", ALL_NAMES)
def test_every_case_takes_its_hand_written_function(name):
    """no case passes its contracts on a stock fall-back: the graph of its output holds the node of the layer's own autograd.Function"""
    want = [fn for prefix, fn in FUNCTIONS if name.startswith(prefix)]
    assert len(want) == 1, (name, want)
    r = AC.Run(cases()[name], DEV)
    seen, todo = set(), [r.y.grad_fn]
    while todo and len(seen) < 64:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        todo += [n for n, _ in node.next_functions]
    names = {type(n).__name__ for n in seen}
    assert want[0] + "Backward" in names, (name, sorted(names))
    if name.endswith("_out_slice_cat"):
        assert "_CatSlicesFnBackward" in names


@pytest.mark.parametrize("name,want", [("subm_128_128_sorted_s16", True), ("subm_128_128_unsorted_s16", False)])
def test_the_sorted_rows_cases_keep_their_mode_in_the_backward(name, want, monkeypatch):
    """control: the sorted-row form is chosen again at backward time from a global (hip_ops.spconv_s16_sorted_ok), so the case's scope must
    hold there too - the forward AND the data gradient of the `sorted` case run hip_ops.spconv_s16_run_sorted, those of `unsorted` never"""
    from sparse2dense_amd import hip_ops as H
    tags, real, before = [], H.spconv_s16_run_sorted, H.SORTED_ROWS

    def spy(*args, **kw):
        tags.append(kw.get("tag", args[7] if len(args) > 7 else "fwd"))
        return real(*args, **kw)
    monkeypatch.setattr(H, "spconv_s16_run_sorted", spy)
    case = cases()[name]
    r = AC.Run(case, DEV)
    n_fwd = len(tags)
    G = case.grad_like(r.y.detach(), 0)
    r.backward(G, retain=True)
    n_bwd = len(tags) - n_fwd
    r.backward(G)
    assert (n_fwd, n_bwd, len(tags) - n_fwd - n_bwd) == ((1, 1, 1) if want else (0, 0, 0)), tags
    assert H.SORTED_ROWS == before   # (the scope put the global back)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_a_masks(name):
    case = cases()[name]
    side = _side()
    AC.contract_masks(case, DEV, modes=[("side stream", side_all) + (((lambda: side.stats["side"]),) if case.uses_side else ())])


@pytest.mark.parametrize("name", ALL_NAMES)
def test_b_upstream_gradient_forms(name):
    AC.contract_grad_forms(cases()[name], DEV)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_c_replay(name):
    AC.contract_replay(cases()[name], DEV)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_d_interleaving_and_accumulation(name):
    case, side = cases()[name], _side()
    AC.contract_interleave(case, DEV)
    AC.contract_accumulate(case, DEV)
    AC.contract_accumulate(case, DEV, mode=side_all, counter=(lambda: side.stats["plain"]) if case.uses_side else None,
                           used=(lambda: side.stats["side"]) if case.uses_side else None)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_e_grad_mode(name):
    AC.contract_grad_mode(cases()[name], DEV)


def _raw_write(p, values):
    p.data.copy_(values)   # through .data: the version counter does not move (what the fused optimizer's raw-pointer update looks like)


@pytest.mark.parametrize("name", LINEAR_NAMES)
def test_f_parameter_updates(name, monkeypatch):
    case, D = cases()[name], _D()
    monkeypatch.setenv("S2D_PACK_GRAPH", "0")
    if case.repack:
        AC.contract_param_update(case, DEV, refresh=D.refresh_pack_cache, raw_write=_raw_write)
    else:
        AC.contract_param_update(case, DEV)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_g_fanout(name):
    AC.contract_fanout(cases()[name], DEV)


def test_eval_batch_norm_cache_of_a_frozen_affine_against_the_trainable_path():
    """the distillation teacher: eval mode, affine frozen -> _BNRowFn's [mean, invstd, scale, shift] cache (the `_frozen` cases run every
    contract on it).  Here the cache against the path without it: same bits, a hit equals the first forward, and it follows an update."""
    for c in (8, 64):
        case = bn2d_case(c, 1, False)
        with AC._recording(case, "cache"):
            full = AC.Run(case, DEV, mask={"x"})
            assert getattr(full.module, "_s2d_eval_fin", None) is not None
            G = case.grad_like(full.y.detach(), 0)
            g = full.backward(G)
            yref, gref = full.reference(G)
            AC._require_close(case, "a", "y", full.y, yref, "frozen affine, eval")
            AC._require_close(case, "a", "x", g["x"], gref["x"], "frozen affine, eval")
            assert g["gamma"] is None and g["beta"] is None
            trainable = AC.Run(case, DEV)
            assert getattr(trainable.module, "_s2d_eval_fin", None) is None
            AC._require_bits(case, "a", "y", trainable.y, full.y, "trainable affine (no cache) vs frozen affine (cache)")
            AC._require_bits(case, "a", "x", trainable.backward(G)["x"], g["x"], "dx: trainable affine vs frozen affine")
            m = full.module
            again = AC.Run(case, DEV, mask={"x"}, module=m)      # second forward: the cache hit
            AC._require_bits(case, "a", "y", again.y, full.y, "cache hit vs first forward")
            with torch.no_grad():
                m.weight.mul_(2); m.bias.mul_(2)
            doubled = AC.Run(case, DEV, mask={"x"}, module=m)
            fresh = case.build(DEV)
            with torch.no_grad():
                fresh.weight.mul_(2); fresh.bias.mul_(2)
            AC._require_bits(case, "f", "y", doubled.y, AC.Run(case, DEV, mask={"x"}, module=fresh).y, "after the frozen affine was updated in place vs a fresh module")


# ----------------------------------------------------------------------------------------------------------------------------------
# producer -> batch norm pairs (fuse_bn_relu sets emit_bn_stats on the producer)
def _bn_train_ref(eps, relu):
    return lambda z, g, b: (torch.relu if relu else (lambda t: t))(F.batch_norm(z, None, None, g, b, True, 0.0, eps))


def _running_ref(z, before):
    dims = [d for d in range(z.dim()) if d != 1]
    n = z.numel() // z.shape[1]
    return {"running_mean": 0.9 * before["running_mean"] + 0.1 * z.mean(dims),
            "running_var": 0.9 * before["running_var"] + 0.1 * z.var(dims, unbiased=False) * n / (n - 1)}


def pair_case(kind):
    """producer -> batch norm, wired as the owners wire them (fuse_bn_relu / emit_bn_stats)"""
    D = _D()
    counter = lambda: D.STATS.get("bn_fwd_folded", 0)
    running = lambda norm: {"running_mean": norm.running_mean, "running_var": norm.running_var}
    nparams = lambda norm: {"gamma": norm.weight, "beta": norm.bias}
    # running statistics: the bound of y, relative to the update this forward made (momentum * (batch statistic - resting value))
    tol = {"y": TBN["y"], "z": TBN["x"], "gamma": TBN["gamma"], "beta": TBN["beta"], "running": TBN["y"]}
    if kind in ("conv3x3", "conv1x1", "conv2x2s2", "convt4x4s2"):
        make, cin, hw = {"conv3x3": (lambda: D.Conv3x3(64, 64, 3, 1, 1, bias=False), 64, (6, 5)),
                         "conv1x1": (lambda: D.Conv1x1(64, 128, 1, bias=False), 64, (6, 5)),
                         "conv2x2s2": (lambda: D.Conv2x2S2(64, 64, 2, 2), 64, (8, 6)),
                         "convt4x4s2": (lambda: D.ConvT4x4S2(128, 64, 4, 2, 1), 128, (6, 5))}[kind]

        def build(device):
            torch.manual_seed(37)
            conv = make()
            norm = D.FastBatchNorm2d(conv.out_channels, eps=1e-3, momentum=0.1)
            conv, norm, _ = D.fuse_bn_relu([conv, norm, torch.nn.ReLU()])
            assert conv.emit_bn_stats and norm.fused_relu
            conv, norm = conv.to(device).train(), norm.to(device).train()
            with torch.no_grad():
                conv.weight.copy_(rb(conv.weight))
                norm.weight.uniform_(0.5, 1.5); norm.bias.uniform_(-0.5, 0.5)
            return conv, norm
        return AC.PairCase(f"{kind}_bn_relu", build, lambda s, d: nhwc16(_randn((2, cin) + hw, s).to(d)), lambda conv, x: conv(x),
                           lambda norm, z: norm(z), nparams, _bn_train_ref(1e-3, True), running, _running_ref, counter, tol, context=autocast, sync=_sync)
    if kind == "subm_s16":
        from sparse2dense_amd import spconv as S
        from sparse2dense_amd import hip_ops as H

        def build(device):
            torch.manual_seed(37)
            conv, norm = S.SubMConv3d(64, 64, 3, padding=1, bias=False, indice_key="k").to(device).train(), S.FeatureBatchNorm1d(64, eps=1e-3, momentum=0.1).to(device).train()
            conv.emit_bn_stats = True   # (as SparseSequential sets it for a conv in front of a FeatureBatchNorm1d)
            with torch.no_grad():
                conv.weight.copy_(rb(conv.weight))
                norm.weight.uniform_(0.5, 1.5); norm.bias.uniform_(-0.5, 0.5)
            return conv, norm

        @contextlib.contextmanager
        def context():
            prev = H.SPARSE_COMPUTE_DTYPE
            H.set_sparse_compute_dtype("s16")
            try:
                yield
            finally:
                H.set_sparse_compute_dtype(prev)

        def inputs(seed, device):
            idx = _sparse_indices(device)
            return _randn((idx.shape[0], 64), seed).to(device).to(torch.bfloat16)
        return AC.PairCase("subm_s16_bn1d_relu", build, inputs, lambda conv, x: conv(S.SparseConvTensor(x, _sparse_indices(x.device), GRID, 2)).features,
                           lambda norm, z: norm(z, relu=True), nparams, _bn_train_ref(1e-3, True), running, _running_ref, counter, tol,
                           context=context, sync=_sync)
    assert kind == "convt3d"
    from sparse2dense_amd import dense3d as D3
    # tests/test_dense3d_gpu.py batch-norm test: outputs 1e-4, gradients 1e-3 of max
    tol3 = {"y": 1e-4, "z": 1e-3, "gamma": 1e-3, "beta": 1e-3, "running": 1e-4}

    def build(device):
        torch.manual_seed(37)
        conv, norm = D3.ConvTranspose3dK4S2(16, 3, 4, 2, 1).to(device).train(), D3.FastBatchNorm3d(3, eps=1e-5, momentum=0.1, fused_relu=True).to(device).train()
        conv.emit_bn_stats = True
        with torch.no_grad():
            norm.weight.uniform_(0.5, 1.5); norm.bias.uniform_(-0.5, 0.5)
        return conv, norm
    return AC.PairCase("convt3d_bn3d_relu", build, lambda s, d: _randn((2, 16, 2, 3, 4), s).to(d), lambda conv, x: conv(x), lambda norm, z: norm(z),
                       nparams, _bn_train_ref(1e-5, True), running, _running_ref, counter, tol3, sync=_sync)


@pytest.mark.parametrize("op", list(AC.INPLACE_OPS))
@pytest.mark.parametrize("kind", ["conv3x3", "conv1x1", "conv2x2s2", "convt4x4s2", "subm_s16", "convt3d"])
def test_h_stale_tags(kind, op):
    AC.contract_stale_tags(pair_case(kind), DEV, op)


@pytest.mark.parametrize("fold", [0, 1, 2])
@pytest.mark.parametrize("kind", ["conv3x3", "conv1x1"])
def test_g_fanout_of_a_batch_norm_output_into_a_conv(kind, fold, monkeypatch):
    """norm -> conv with the norm's output also feeding an identity skip.  With BN_BWD_FOLD the conv's data gradient carries the norm's
    backward sums as a tag, and autograd adds the skip's gradient to that very gradient: the sums of the conv's term alone must not be
    taken for the total.  Reference: the norm's float64 backward over the upstream gradient it really received (the conv's data
    gradient, from a run cut between the two layers, plus the skip's), at the norm's own tolerances."""
    D = _D()
    monkeypatch.setattr(D, "BN_BWD_FOLD", fold)
    pad = 1 if kind == "conv3x3" else 0

    def build(device):
        torch.manual_seed(41)
        norm = D.FastBatchNorm2d(64, eps=1e-3, momentum=0.1, fused_relu=True)
        conv = D.Conv3x3(64, 64, 3, 1, 1, bias=False) if kind == "conv3x3" else D.Conv1x1(64, 128, 1, bias=False)
        m = torch.nn.Sequential(norm, conv).to(device).train()
        with torch.no_grad():
            norm.weight.uniform_(0.5, 1.5); norm.bias.uniform_(-0.5, 0.5); conv.weight.copy_(rb(conv.weight))
        return m

    def call(m, i):
        i["a"] = m[0](i["x"])
        return m[1](i["a"])

    def ref(o):
        a = torch.relu(F.batch_norm(o["x"], None, None, o["gamma"], o["beta"], True, 0.0, 1e-3))
        a = a.detach().to(torch.bfloat16).double() + (a - a.detach())   # the conv reads the bf16-stored activation
        return F.conv2d(a, o["weight"], padding=pad)
    tol = dict(TBN, weight=2e-3)
    case = AC.Case(f"bn_relu_{kind}_fold{fold}", build, lambda s, d: {"x": nhwc16((_randn((2, 64, 6, 5), s) * 1.5 + 0.3).to(d))}, call,
                   lambda m: {"gamma": m[0].weight, "beta": m[0].bias, "weight": m[1].weight}, ref, tol, context=autocast, has_stats=True, sync=_sync)

    def norm_reference(run, upstream):
        ops = {k: run.leaf[k].detach().double().cpu().requires_grad_(True) for k in ("x", "gamma", "beta")}
        an = torch.relu(F.batch_norm(ops["x"], None, None, ops["gamma"], ops["beta"], True, 0.0, 1e-3))
        gs = torch.autograd.grad(an, [ops["x"], ops["gamma"], ops["beta"]], upstream.double().cpu())
        return dict(zip(("x", "gamma", "beta"), gs))

    with AC._recording(case, "g_mid"):
        # the conv's data gradient on its own: a run cut between the layers (the detached tensor carries no tag)
        cut = AC.Run(case, DEV)
        G = case.grad_like(cut.y.detach(), 0)
        m = case.build(DEV)
        x = case.inputs(0, DEV)["x"]
        with autocast():
            a_cut = m[0](x).detach().requires_grad_(True)
            m[1](a_cut).backward(G)
        _sync()
        da = a_cut.grad
        # control: no skip - with the fold on, the sums from the conv's epilogue are consumed
        folded0 = D.STATS["bn_bwd_folded"]
        ga = cut.backward(G)
        assert D.STATS["bn_bwd_folded"] == folded0 + (1 if fold else 0), "control: the conv's epilogue sums feed the norm's backward when nothing else reads its output"
        want = norm_reference(cut, da)
        for k in want:
            AC._require_close(case, "g", k, ga[k], want[k], "no skip")
        AC._require_bits(case, "g", "weight", ga["weight"], m[1].weight.grad, "conv weight gradient: whole chain vs cut run")
        # the skip: a second consumer of the norm's output
        r = AC.Run(case, DEV)
        a = r.inputs["a"]
        Gskip = AC.default_grad(a.detach(), 5)
        folded1 = D.STATS["bn_bwd_folded"]
        torch.autograd.backward([r.y, a * 1], [G, Gskip])
        _sync()
        assert D.STATS["bn_bwd_folded"] == folded1, "sums of the conv's data gradient alone were taken for a gradient that has a second term"
        want = norm_reference(r, da + Gskip)
        for k in want:
            AC._require_close(case, "g", k, r.leaf[k].grad, want[k], "with an identity skip at the norm's output")
        AC._require_bits(case, "g", "weight", r.leaf["weight"].grad, ga["weight"], "conv weight gradient with the skip vs without")
    AC.contract_fanout(case, DEV, label=f"_fold{fold}")
