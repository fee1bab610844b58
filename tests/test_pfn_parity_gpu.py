"""Float64 parity of every entry of csrc/pfn.hip (the fused PointPillars feature net: the one-layer reader's 3 kernels, the two-layer
reader's 4 kernels, 13 entries), called through _lib.load() with raw pointers as sparse2dense_amd/pillars.py calls them.  References,
bounds, checkers and case tables: tests/pfn_ref.py (its docstring derives every bound); tests/test_pfn_checks_cpu.py shows on the host
that each checker can fail and that the committed seeds meet the strict-argmax and redraw conditions.

Every launch writes caller-owned, NaN-filled outputs between guard rows (uint8 outputs: 0xEE), reads inputs that sit between poisoned
fences of their own (the fence of coors is a whole number of rows: it is read as int4), sizes partial buffers from s2d_pfn_blocks,
s2d_pfn_bwd_cols, s2d_pfn2_bwd_rows and s2d_pfn2_bwd_cols only, and runs twice: every element written, every guard intact, the second
launch bit-equal, then the parity checks.

Axes (pfn_ref.CASES): slots T in 1, 2, 12, 13, 19, 20 (12 | 13 straddle the 64-float lane boundary of pfn2_fetch, 1 leaves the second
half-wave idle, 19 | 20 reach the full pillar with num and coors in the spare lanes) at P = 5 and 4097; pillars P in 1, 3, 4, 5, 1023,
1025, 4096, 4097, 9001 (idle waves in a block, idle waves among the backward's 1024, exactly 1024 full blocks, one wave round twice,
ragged multiple trips) at T = 13 and 20.  num_points is forced to 0, 1, T, T + 3 and -1 on about half of the pillars; every fourth pillar
repeats one point (exact ties); half the channels have a positive shift (maxima in an empty slot), every fourth a negative scale, two
channels are all zero (slot 0 must win).  The backward entries get the float64 first maximum, the first empty slot, a later empty
slot, T - 1 everywhere and 0 everywhere as their argmax; pfn2_bwd a training-style and an eval-style abd2."""
import functools
import os
import types

import pytest
import torch

import pfn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
BWD_VARIANTS = (("valid", "train"), ("valid", "eval"), ("n", "train"), ("above_n", "eval"), ("last", "train"), ("zero", "eval"))
BYTE_FILL = 0xEE
SHARES = {}
nan_bits = torch.tensor(float("nan")).view(torch.int32).item()


@functools.lru_cache(maxsize=None)
def _lib():
    from sparse2dense_amd import _lib as L
    return L.load()


def call(name, *args):
    return int(R.entry(_lib(), name)(*args))


def ok(name, *args):
    rc = call(name, *args)
    if rc != 0:
        from sparse2dense_amd import _lib as L
        raise AssertionError(f"{name} returned {rc}: {L.last_error()}")


def stream():
    return torch.cuda.current_stream().cuda_stream


def fenced(t):
    """a device copy of the host tensor t [rows, ...] between R.GUARD poisoned rows on each side -> (allocation, the copy)"""
    fill = float("nan") if t.dtype.is_floating_point else (0x7F if t.dtype == torch.uint8 else 0x7F7F7F7F)
    buf = torch.full((t.shape[0] + 2 * R.GUARD,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=DEV)
    buf[R.GUARD:-R.GUARD] = t.to(DEV)
    return buf, buf[R.GUARD:-R.GUARD]


def fence_all(ns, names):
    """the namespace with its tensors `names` replaced by fenced device copies; the allocations stay alive in .allocs"""
    out = types.SimpleNamespace(**vars(ns))
    out.allocs = {}
    for k in names:
        out.allocs[k], view = fenced(getattr(ns, k))
        setattr(out, k, view)
    return out


def fences_intact(ns):
    for k, buf in ns.allocs.items():
        ref = torch.full_like(buf[:R.GUARD], float("nan") if buf.dtype.is_floating_point else 0x7F7F7F7F)
        for g in (buf[:R.GUARD], buf[-R.GUARD:]):
            assert bool((g.contiguous().view(torch.int32) == ref.contiguous().view(torch.int32)).all()), f"the fence of input {k} was overwritten"


@functools.lru_cache(maxsize=None)
def params():
    host = R.make_params()
    prm = fence_all(host, ("w", "scale", "shift", "w1", "w2", "ss1", "ss2"))
    prm.abd2 = {}
    for k, v in host.abd2.items():
        prm.allocs["abd2 " + k], prm.abd2[k] = fenced(v)
    return host, prm


@functools.lru_cache(maxsize=None)
def setup(p, t):
    host, prm = params()
    case = fence_all(R.screened_case(p, t, host, DEV), ("vox", "num", "coors"))
    case.dup = case.dup.to(DEV)
    assert case.allocs["coors"].data_ptr() % 16 == 0 and case.coors.data_ptr() % 16 == 0
    blocks = call("s2d_pfn_blocks", p)
    assert blocks == R.blocks_mirror(p), (blocks, R.blocks_mirror(p))
    return case, prm, blocks


def head(case, w):
    return (case.vox.data_ptr(), case.num.data_ptr(), case.coors.data_ptr(), w.data_ptr())


def geo(case):
    return (case.P, case.T, 5, *case.geo)


def byte_rows(rows):
    buf = torch.full((rows + 2 * R.GUARD, R.C), BYTE_FILL, dtype=torch.uint8, device=DEV)
    return buf, buf[R.GUARD:-R.GUARD]


def byte_rows_ok(buf, slots, what):
    assert bool((buf[:R.GUARD] == BYTE_FILL).all()) and bool((buf[-R.GUARD:] == BYTE_FILL).all()), f"{what}: guard rows overwritten"
    assert bool((buf[R.GUARD:-R.GUARD] < slots).all()), f"{what}: elements left at the fill or not a slot"


def twice(launch, what, case, prm):
    """launch() -> [(allocation, view)] per output; run twice into fresh poisoned outputs: all written, guards and input fences intact,
    bit-equal -> the views of the first run"""
    runs = []
    for _ in range(2):
        outs = launch()
        torch.cuda.synchronize()
        for i, (buf, view) in enumerate(outs):
            if buf.dtype == torch.uint8:
                byte_rows_ok(buf, case.T, f"{what}, output {i}")
            else:
                R.assert_written(buf, f"{what}, output {i}")
        runs.append([v for _, v in outs])
    fences_intact(case)
    fences_intact(prm)
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.uint8 else a.view(torch.int32),
                           b.view(torch.uint8) if b.dtype == torch.uint8 else b.view(torch.int32)), f"{what}, output {i}: the second launch differs"
    return runs[0]


def partial(rows, *shape):
    return R.poisoned(rows, *shape, dtype=F32, device=DEV)


def test_support_and_size_queries():
    lib = _lib()
    for t in range(0, 23):
        want = int(1 <= t <= R.T_MAX)
        assert call("s2d_pfn_supported", 5, t, R.F, R.C) == want and call("s2d_pfn2_supported", 5, t, R.F, R.C1, R.C) == want, t
    assert call("s2d_pfn_supported", 4, 20, R.F, R.C) == 0 and call("s2d_pfn2_supported", 5, 20, R.F, R.C, R.C) == 0
    for p in R.P_AXIS + (1 << 20,):
        assert call("s2d_pfn_blocks", p) == R.blocks_mirror(p), p
    assert call("s2d_pfn_bwd_cols") == R.BWD_COLS and call("s2d_pfn2_bwd_cols") == R.BWD2_COLS and call("s2d_pfn2_bwd_rows") == R.BWD2_ROWS
    assert lib is not None


@pytest.mark.parametrize("p,t", R.CASES)
def test_one_layer_reader(p, t):
    """pfn_stats, pfn_apply_max and pfn_bwd (five argmax kinds) of one case"""
    case, prm, blocks = setup(p, t)
    ref = R.Ref1(case, prm)
    fam = "pfn"

    def stats():
        out = partial(blocks, 2, R.C)
        ok("s2d_pfn_stats_f32", *head(case, prm.w), *geo(case), out[1].data_ptr(), stream())
        return [out]
    (slab,) = twice(stats, "pfn_stats", case, prm)
    R.check_rows(slab, *ref.stats(blocks), "pfn_stats", f"{fam}_stats", "block, sum, channel")

    def apply():
        out, arg = partial(p, R.C), byte_rows(p)
        ok("s2d_pfn_apply_max_f32", *head(case, prm.w), prm.scale.data_ptr(), prm.shift.data_ptr(), *geo(case), out[1].data_ptr(), arg[1].data_ptr(), stream())
        return [out, arg]
    out, arg = twice(apply, "pfn_apply_max", case, prm)
    y, ey = ref.apply()
    share = R.check_argmax(y, ey, ref.part, out, arg, "pfn_apply_max", f"{fam}_apply_max")
    SHARES[("pfn_apply_max", p, t)] = share

    first = R.first_max(y, ref.part)[1]
    cols = call("s2d_pfn_bwd_cols")
    g_alloc, g = fenced(R.make_grad(case, 21, "cpu"))
    for kind in R.ADVERSARIAL_ARG:
        a_alloc, a = fenced(R.make_arg(case, kind, first).cpu())

        def bwd():
            out = partial(blocks, cols)
            ok("s2d_pfn_bwd_f32", *head(case, prm.w), g.data_ptr(), a.data_ptr(), *geo(case), out[1].data_ptr(), stream())
            return [out]
        (rows,) = twice(bwd, f"pfn_bwd, arg {kind}", case, prm)
        R.check_bwd_rows(rows, *ref.bwd(a, g, blocks), f"pfn_bwd, arg {kind}", f"{fam}_bwd")
        for fence in (a_alloc[:R.GUARD], a_alloc[-R.GUARD:]):
            assert bool((fence == 0x7F).all()), "the fence of the argmax input was overwritten"
        for fence in (g_alloc[:R.GUARD], g_alloc[-R.GUARD:]):
            assert bool((fence.view(torch.int32) == nan_bits).all()), "the fence of the gradient input was overwritten"


@pytest.mark.parametrize("p,t", R.CASES)
def test_two_layer_reader(p, t):
    """pfn2_stats1, pfn2_stats2, pfn2_apply_max and pfn2_bwd (argmax kinds x training- and eval-style abd2) of one case"""
    case, prm, blocks = setup(p, t)
    ref = R.Ref2(case, prm)
    assert not bool(ref.rejected().any()), "the screening left a pillar whose layer-1 decisions fp32 could take differently"
    fam = "pfn2"
    w12 = head(case, prm.w1) + (prm.w2.data_ptr(), prm.ss1.data_ptr())

    def stats1():
        out = partial(blocks, 2, R.C)
        ok("s2d_pfn2_stats1_f32", *head(case, prm.w1), *geo(case), out[1].data_ptr(), stream())
        return [out]
    (slab,) = twice(stats1, "pfn2_stats1", case, prm)
    R.check_rows(slab, *ref.stats1(blocks), "pfn2_stats1", f"{fam}_stats1", "block, sum, channel")

    def stats2():
        out = partial(blocks, 2, R.C)
        ok("s2d_pfn2_stats2_f32", *w12, *geo(case), out[1].data_ptr(), stream())
        return [out]
    (slab,) = twice(stats2, "pfn2_stats2", case, prm)
    R.check_rows(slab, *ref.stats2(blocks), "pfn2_stats2", f"{fam}_stats2", "block, sum, channel")

    def apply():
        out, arg, h2m = partial(p, R.C), byte_rows(p), partial(p, R.C)
        ok("s2d_pfn2_apply_max_f32", *w12, prm.ss2.data_ptr(), *geo(case), out[1].data_ptr(), arg[1].data_ptr(), h2m[1].data_ptr(), stream())
        return [out, arg, h2m]
    out, arg, h2max = twice(apply, "pfn2_apply_max", case, prm)
    y, ey = ref.apply()
    share = R.check_argmax(y, ey, ref.part, out, arg, "pfn2_apply_max", f"{fam}_apply_max", ref.h2, ref.eh2, h2max)
    SHARES[("pfn2_apply_max", p, t)] = share

    first = R.first_max(y, ref.part)[1]
    rows_n, cols = call("s2d_pfn2_bwd_rows"), call("s2d_pfn2_bwd_cols")
    assert rows_n == R.BWD2_ROWS and cols == R.BWD2_COLS
    g_alloc, g = fenced(R.make_grad(case, 22, "cpu"))
    for kind, abd in BWD_VARIANTS:
        a_alloc, a = fenced(R.make_arg(case, kind, first).cpu())

        def bwd():
            out = partial(rows_n, cols)
            ok("s2d_pfn2_bwd_f32", *w12, prm.abd2[abd].data_ptr(), g.data_ptr(), a.data_ptr(), *geo(case), out[1].data_ptr(), stream())
            return [out]
        what = f"pfn2_bwd, arg {kind}, abd2 {abd}"
        (rows,) = twice(bwd, what, case, prm)
        R.check_bwd_rows(rows, *ref.bwd(a, g, prm.abd2[abd]), what, f"{fam}_bwd")
        for fence in (a_alloc[:R.GUARD], a_alloc[-R.GUARD:]):
            assert bool((fence == 0x7F).all()), "the fence of the argmax input was overwritten"
        for fence in (g_alloc[:R.GUARD], g_alloc[-R.GUARD:]):
            assert bool((fence.view(torch.int32) == nan_bits).all()), "the fence of the gradient input was overwritten"


MODULE_CASES = [(filters, train, p, t) for filters in ((64,), (64, 64)) for train in (True, False) for p in (1, 5, 4101) for t in (13, 20)]
MODULE_ROUNDS = {}
MODULE_REL = {}     # family -> the largest median of bound / |reference| over its cases


@pytest.mark.parametrize("filters,train,p,t", MODULE_CASES)
def test_module_on_top_of_the_entries(filters, train, p, t):
    """PillarFeatureNet through _FusedPfnFn / _FusedPfn2Fn: the slab folds, the [:, :32] column selections, the batch-norm finalisation,
    dW = a M1 + b M2 + d M3 and the eval shortcuts.  The float64 reference takes the kernel's saved arg for the last maximum (a
    gather), so every element of out, of every parameter gradient and of the running statistics is held to its propagated bound
    (pfn_ref.ModuleRef).  The two-layer reader's inputs are screened as for pfn2_bwd; a layer-1 shift within the margin of the ReLU's
    zero is moved by 0.05 through the layer's bias.  In train mode at P = 4101 the redraw loop cannot empty (see below): there, and
    wherever a pre-activation lies within its own bound of zero (out > 0 in the backward), the bounds carry both outcomes of the
    decision.  For the two-layer reader in train mode the first layer's gradient bounds are vacuous (pfn_ref's docstring derives
    why); the report prints the median relative bound per family.  The redraw loop stops at its cap.  P = 1 pins the squeezed shape."""
    from sparse2dense_amd.pillars import PillarFeatureNet
    torch.manual_seed(3)
    net = PillarFeatureNet(num_input_features=5, num_filters=filters, voxel_size=(0.32, 0.32, 6.0), pc_range=(-74.88, -74.88, -2, 74.88, 74.88, 4.0))
    with torch.no_grad():
        net.pfn_layers[0].linear.weight.mul_(0.3)
        for lyr in net.pfn_layers:
            c = lyr.units
            lyr.norm.weight.copy_(torch.rand(c) + 0.5)
            lyr.norm.weight[1::4] *= -1.0
            lyr.norm.bias.copy_(torch.randn(c) * 0.5)
            lyr.norm.running_mean.copy_(torch.randn(c) * 0.1)
            lyr.norm.running_var.copy_(torch.rand(c) + 0.5)
    net = net.train(train).to(DEV)
    assert net._fused_ok(torch.zeros(1, t, 5, device=DEV)) == len(filters), "the fused reader was not selected"
    assert (R.f32(net.vx), R.f32(net.vy), R.f32(net.x_offset), R.f32(net.y_offset)) == R.GEO

    def snapshot():
        return [types.SimpleNamespace(w=l.linear.weight.detach().clone(), gamma=l.norm.weight.detach().clone(), beta=l.norm.bias.detach().clone(),
                                        rm=l.norm.running_mean.clone(), rv=l.norm.running_var.clone(), eps=l.norm.eps, momentum=l.norm.momentum)
                  for l in net.pfn_layers]

    host = R.make_case(p, t, seed=R.seed_of(p, t) + 7)
    for rnd in range(1, R.REDRAW_ROUNDS + 1):
        case = R.case_to(host, DEV)
        layers = snapshot()
        mref = R.ModuleRef(case, layers, train)
        running = mref.forward()
        if len(filters) == 1 or (train and p > 5):
            # the one-layer backward recomputes no decision.  Batch statistics over thousands of pillars: every redraw moves all the
            # pre-activations by more than the margin and the loop cannot empty; the bounds then carry the layer-1 decisions that may
            # fall either way (pfn_ref.Ref2.bwd), as they carry out > 0 in every case (ModuleRef.backward)
            break
        pillars, shift1 = mref.ambiguous()
        if bool(shift1.any()):
            with torch.no_grad():
                net.pfn_layers[0].norm.bias[shift1] += 0.05
        bad = pillars.cpu()
        if not bool(shift1.any()) and not bool(bad.any()):
            break
        if bool(bad.any()):
            R._draw_points(host, bad.nonzero().flatten(), host.gen)
    # unlike the entry-level cases, a loop that reaches its cap is no failure here: a decision within the margin but outside its own
    # bound is the float64 one anyway, and one inside its bound is carried by the bounds.  The report prints the rounds used
    else:
        case, layers = R.case_to(host, DEV), snapshot()      # the last round redrew: the reference of what the module gets
        mref = R.ModuleRef(case, layers, train)
        running = mref.forward()
    MODULE_ROUNDS[(filters, train, p, t)] = rnd

    dout = R.make_grad(case, 33, DEV)
    out = net(case.vox, case.num, case.coors)
    assert tuple(out.shape) == ((R.C,) if p == 1 else (p, R.C))      # .squeeze(), as the layer-by-layer path
    fn = out.grad_fn
    while not type(fn).__name__.startswith("_FusedPfn"):
        fn = fn.next_functions[0][0]
    arg = fn.saved_tensors[-1 if len(filters) == 1 else -2]
    assert arg.dtype == torch.uint8 and tuple(arg.shape) == (p, R.C)
    out.backward(dout.view_as(out))
    torch.cuda.synchronize()
    mref.check_out(out.detach().view(p, R.C), arg)
    grads = mref.backward(arg, dout)
    names = [n for n, _ in net.named_parameters()]
    assert sorted(names) == sorted(grads), (names, sorted(grads))
    for name, prm in net.named_parameters():
        fam = f"module, {len(filters)} layer(s), {'train' if train else 'eval'}: d {name[len('pfn_layers.'):]}"
        R.check_rows(prm.grad, *grads[name], f"module: gradient of {name}", fam, "index")
        ref, bound = grads[name]
        MODULE_REL[fam] = max(MODULE_REL.get(fam, 0.0), float((bound / ref.abs().clamp_min(1e-30)).median()))
    buffers = dict(net.named_buffers())
    for i, (l, before) in enumerate(zip(net.pfn_layers, layers)):
        if train:
            for which in ("running_mean", "running_var"):
                name = f"pfn_layers.{i}.norm.{which}"
                R.check_rows(buffers[name], *running[name], f"module: {name}", "module " + which, "channel")
            assert int(l.norm.num_batches_tracked) == 1
        else:
            assert torch.equal(l.norm.running_mean, before.rm) and torch.equal(l.norm.running_var, before.rv) and int(l.norm.num_batches_tracked) == 0


def _whole_file_selected(request):
    here = request.node.module
    selected = {it.originalname for it in request.session.items if getattr(it, "module", None) is here}
    return {k for k, v in vars(here).items() if k.startswith("test_") and callable(v)} <= selected


def report_lines():
    lines = ["family                                                              worst |error| / bound"]
    lines += [f"{k:<68s}{v:.3f}" for k, v in sorted(R.WORST.items()) if k.startswith("pfn")]
    lines += ["", "smallest share of (pillar, channel) pairs under the strict first-maximum rule"]
    for name in ("pfn_apply_max", "pfn2_apply_max"):
        vals = [v for (n, _, _), v in SHARES.items() if n == name]
        if vals:
            lines.append(f"{name:<68s}{min(vals):.4f}")
    if MODULE_ROUNDS:
        lines += ["", f"module test: screening rounds used, largest of {len(MODULE_ROUNDS)} cases: {max(MODULE_ROUNDS.values())} (cap {R.REDRAW_ROUNDS})"]
    if MODULE_REL:
        lines += ["", "module test: median bound / |reference| per family (largest over the cases)"]
        lines += [f"{k:<68s}{v:.2e}" for k, v in sorted(MODULE_REL.items())]
    lines += ["", f"entries called: {len(R.CALLED)} of {len(R.table_entries())}"]
    return lines


def test_every_entry_was_called_and_report(request, capsys):
    """the last test of the file: prints the worst |error| / bound per family (profiles/pfn_parity.txt is such a print; with
    PFN_PARITY_REPORT=<path> it is also written there).  Every figure in it has passed its check already"""
    assert R.CALLED <= R.table_entries()
    if _whole_file_selected(request):
        assert R.CALLED == R.table_entries(), ("entries that no case reached", sorted(R.table_entries() - R.CALLED))
    with capsys.disabled():
        print("\n" + "\n".join(report_lines()))
    path = os.environ.get("PFN_PARITY_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(report_lines()) + "\n")
