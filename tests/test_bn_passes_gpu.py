"""Float64 parity of every batch-norm pass entry of csrc/features.hip (s2d_bn1d_*, s2d_bnrow_*, s2d_bncm_*, s2d_bn_partials_*), called
through _lib.load() with raw pointers, at every edge of the launch plans.  References, plan mirrors, bounds and checkers:
tests/bn_pass_ref.py (its docstring derives every bound); tests/test_bn_pass_checks_cpu.py shows that the checkers can fail.

Every case first asserts that the mirrored plan is the one the library takes (the *_workspace_bytes query), runs each entry with a
workspace of exactly the queried size between poisoned guards under both poison bytes (bit-equal results), into NaN-filled,
guarded outputs, and asserts that no ReLU mask recomputed from x is ambiguous (no element is ever excluded from a comparison).

Input families: benign (randn * 2 + 0.3), offset (mean / std = 16), and in both: channel 1 = the constant 1.0 with scale 1,
shift -1 (exact zeros of z, variance exactly 0, eps 1e-3 and 1e-5), channel 2 with gamma = scale = a = 0, channel 3 a constant whose
fp32 sums are inexact, channel 4 with |z| up to 10 and beyond (the GELU tails).

Template instantiations the dispatchers can select, and the test that reaches each:
  row_reduce_bf16_kernel<BWD, ACT, HAS_Y>
    <false, 0, false>  test_row_stats, test_row_reduce_cap, test_row_fused_against_split
    <true, 0, false>   test_row_bwd_reduce (act 0)
    <true, 1, true>    test_row_bwd_reduce (act 1, mask from y)
    <true, 1, false>   test_row_bwd_reduce (act 1, mask from x), test_row_reduce_cap
    <true, 2, false>   test_row_bwd_reduce (act 2)
  row_apply_bf16_kernel<RES, ACT>
    <false | true, 0 | 1 | 2>  test_row_apply (residual off / on x act 0 / 1 / 2); <true, 1> also test_row_apply_cap
  row_bwd_apply_bf16_kernel<ACT, HAS_Y, HAS_DRES>
    <0, false, false | true>   test_row_bwd_apply (act 0; dres without an activation is dy)
    <2, false, false | true>   test_row_bwd_apply (act 2)
    <1, true, false | true>    test_row_bwd_apply (act 1, y given)
    <1, false, false | true>   test_row_bwd_apply (act 1, mask from x); <1, false, true> also test_row_apply_cap
  cm_reduce_kernel<true, TX, TG> / cm_apply_kernel<true, TX, TG, TO>
    <float, float[, float]>, <float, bf16[, float]>, <bf16, bf16[, bf16]>   test_cm_typed
  cm_reduce_kernel<false> / <true> and cm_apply_kernel<false> / <true> (fp32)   test_cm
"""
import functools
import os
import types

import pytest
import torch

import bn_pass_ref as R
from ws_guard import POISONS, GuardLog

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
INVSTD = {}   # family -> the worst |invstd - float64| / float64 seen (reported for the offset-mean family)
MEASURED = {}   # "e_act": what test_gelu_yardstick measured in this process


@functools.lru_cache(maxsize=None)
def _lib():
    from sparse2dense_amd import _lib as L
    return L.load()


def call(name, *args):
    return int(R.entry(_lib(), name)(*args))


def ok(name, *args):
    rc = call(name, *args)
    if rc != R.S2D_OK:
        from sparse2dense_amd import _lib as L
        raise AssertionError(f"{name} returned {rc}: {L.last_error()}")


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def f32(v):
    """the fp32 value the entry receives for a float argument"""
    return float(torch.tensor(v, dtype=F32))


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def fvec(n, dtype=F32):
    """a NaN-filled vector of n words between 4 guard words -> (allocation, view)"""
    buf = torch.full((n + 8,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[4:4 + n]


def fvec_ok(buf, written, what):
    body = buf[4:-4]
    assert bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[-4:]).all()), f"{what}: guard words overwritten"
    assert bool(torch.isfinite(body[:written]).all()), f"{what}: words left at the NaN fill"
    assert bool(torch.isnan(body[written:]).all()), f"{what}: words behind the result overwritten"


def with_ws(nbytes, run):
    """run(ws pointer | None, nbytes) -> a tuple of result tensors, once per poison byte, the workspace exactly nbytes long between
    poisoned guards; the guards hold and the two runs agree bit for bit; -> the results"""
    outs = []
    for poison in POISONS:
        log = GuardLog(poison)
        ws = log.alloc("bn_pass", nbytes, DEV)
        outs.append(run(ws.data_ptr() if nbytes else None, nbytes))
        torch.cuda.synchronize()
        log.check()
    for i, (a, b) in enumerate(zip(*outs)):
        R.check_bits(a, b, f"result {i} under the two workspace poisons", "index")
    return outs[0]


class ChanOut:
    """guarded per-channel fp32 outputs of a finalize entry"""

    def __init__(self, names, c, init=None):
        self.names, self.c = names, c
        self.bufs = {k: fvec(c) for k in names}
        for k, v in (init or {}).items():
            self.bufs[k][1].copy_(v)

    def ptr(self, k):
        return p(self.bufs[k][1]) if k in self.bufs else None

    def result(self, what):
        torch.cuda.synchronize()
        for k, (buf, _) in self.bufs.items():
            fvec_ok(buf, self.c, f"{what}: {k}")
        return {k: v.clone() for k, (_, v) in self.bufs.items()}


FWD = ("mean", "invstd", "scale", "shift")
RUN = ("running_mean", "running_var")
BWD = ("dgamma", "dbeta", "a", "b", "d")


def chan_tuple(d):
    return tuple(d[k] for k in sorted(d))


def note_invstd(family, got, fn, s0, s1, n):
    """the observed relative invstd error per input family, at 256 rows or more (below, a random channel can be as ill-conditioned
    as it likes); channels without variance (constant channels, every channel at n = 1: float64 variance below 1e-6 of the mean
    square, invstd = eps^-1/2, ill-conditioned by design) are reported apart"""
    ref = fn(s0, s1)["invstd"][0]
    rel = (got.double() - ref).abs() / ref
    flat = 1.0 - (s0 * s0 / n) / s1.clamp_min(1e-300) < 1e-6   # var / E[x^2]
    for name, sel in ((family if n >= 256 else family + ", fewer than 256 rows", ~flat), ("channels without variance", flat)):
        if bool(sel.any()):
            INVSTD[name] = max(INVSTD.get(name, 0.0), float(rel[sel].max()))


def apart_channels(s, s0, s1, n):
    """channels whose share of the finalize box is reported apart: no variance (the clamp puts invstd on the box's corner) or gamma = 0"""
    return (1.0 - (s0 * s0 / n) / s1.clamp_min(1e-300) < 1e-6) | (s.gamma == 0)


def params(c, family, seed):
    """per-channel fp32 vectors of a case: scale / shift (z centred on the data), a / b / d, gamma / beta, running statistics"""
    g = gen(seed)
    rn = lambda: torch.randn(c, device=DEV, generator=g)
    s = types.SimpleNamespace()
    s.scale = rn() * 0.5 + 1.0
    if c > 4:
        s.scale[4] = 5.0 if family == "benign" else 20.0
    s.shift = rn() * 0.5 - (8.0 * s.scale if family == "offset" else 0.0)
    s.a, s.b, s.d = rn(), rn() * 0.1, rn() * 0.1
    s.gamma, s.beta = rn() * 0.5 + 1.0, rn()
    s.rm, s.rv = rn(), torch.rand(c, device=DEV, generator=g) + 0.5
    if c > 4:
        s.scale[1], s.shift[1] = 1.0, -1.0
        s.scale[2] = s.a[2] = s.gamma[2] = 0.0
    return s


def rows(shape, family, dtype, seed):
    g = gen(seed)
    x = torch.randn(shape, device=DEV, generator=g)
    return (x * 2.0 + 0.3 if family == "benign" else x * 0.5 + 8.0).to(dtype)


@functools.lru_cache(maxsize=4)
def row_case(c, n, family, dtype=BF):
    s = params(c, family, 1000 * c + n)
    s.x = rows((n, c), family, dtype, 7 * c + n)
    if c > 4:
        s.x[:, 1], s.x[:, 3] = 1.0, 0.30078125
    g = gen(c + 31 * n)
    s.dy = torch.randn(n, c, device=DEV, generator=g).to(dtype)
    s.res = torch.randn(n, c, device=DEV, generator=g).to(dtype)
    s.y = torch.randn(n, c, device=DEV, generator=g).clamp_min(0.0).to(dtype)   # a stored forward output: about half exact zeros
    assert R.make_unambiguous(s.x, s.scale, s.shift) == 0
    assert int(R.ambiguous(s.x, s.scale, s.shift).sum()) == 0, "ambiguous ReLU masks left in the input"
    if c > 4:
        z, _ = R.ref_z(s.x[:, 1], s.scale[1], s.shift[1])
        assert bool((z == 0).all()), "channel 1 must hold exact zeros of z"
    # statistics the backward entries take as inputs (any fp32 vectors do; these are the batch's own)
    ref, _ = R.ref_sums(s.x)
    fin = R.fwd_finalize(ref[:c], ref[c:], n, s.gamma, s.beta, f32(1e-3), f32(0.1))
    s.mean, s.invstd = fin["mean"][0].float(), fin["invstd"][0].float()
    return s


def families(ns):
    """(n, family): the benign family at every row count, the offset family at the two largest"""
    return [(n, "benign") for n in ns] + [(n, "offset") for n in ns[-2:]]


def fwd_fn(s, n, eps, mom, running):
    return lambda s0, s1: R.fwd_finalize(s0, s1, n, s.gamma, s.beta, f32(eps), f32(mom), s.rm if running else None, s.rv if running else None)


def bwd_fn(s, n):
    def fn(s0, s1):
        out = R.bwd_finalize_local(s0, s1, s.mean, s.invstd)
        out.update(R.bwd_finalize_global(s0, s1, n, s.gamma, s.mean, s.invstd))
        return out
    return fn


def sums_box(ref, mag, chain, act_sum=None):
    d = chain * R.U32 * mag + (act_sum if act_sum is not None else 0.0)
    c = ref.numel() // 2
    return ref[:c], d[:c], ref[c:], d[c:]


# ======== A. row-major bf16 ==============================================================================================================
def row_plan_checked(n, c):
    plan = R.row_plan_bf16(n, c)
    assert call("s2d_bnrow_workspace_bytes", n, c) == plan.ws_bytes, ("the mirrored row plan is not the one taken", n, c, plan)
    return plan


def run_row_stats(s, n, c, plan, write_count):
    def run(ws, nb):
        buf, st = fvec(2 * c + 2)
        ok("s2d_bnrow_stats_bf16", p(s.x), n, c, p(st), write_count, ws, nb, stream())
        torch.cuda.synchronize()
        fvec_ok(buf, 2 * c + write_count, "bnrow_stats")
        return (st[:2 * c + write_count].clone(),)
    (st,) = with_ws(plan.ws_bytes, run)
    if write_count:
        assert float(st[2 * c]) == float(n), "the count word"
    return st[:2 * c]


def run_row_stats_finalize(s, n, c, plan, eps, mom, running, name="s2d_bnrow_stats_finalize_bf16"):
    def run(ws, nb):
        out = ChanOut(FWD + (RUN if running else ()), c, {"running_mean": s.rm, "running_var": s.rv} if running else None)
        bt = torch.tensor([-7, 5, -7], dtype=torch.int64, device=DEV)
        ok(name, p(s.x), n, c, p(s.gamma), p(s.beta), eps, mom, out.ptr("mean"), out.ptr("invstd"), out.ptr("scale"), out.ptr("shift"),
           out.ptr("running_mean"), out.ptr("running_var"), p(bt[1:]) if running else None, ws, nb, stream())
        res = out.result(name)
        assert bt.tolist() == ([-7, 6, -7] if running else [-7, 5, -7]), "num_batches_tracked"
        return chan_tuple(res)
    names = sorted(FWD + (RUN if running else ()))
    return dict(zip(names, with_ws(plan.ws_bytes, run)))


def check_row_stats(c, n, family):
    s = row_case(c, n, family)
    plan = row_plan_checked(n, c)
    ref, mag = R.ref_sums(s.x)
    for wc in (0, 1):
        st = run_row_stats(s, n, c, plan, wc)
        R.check_sums(st, ref, mag, R.chain_rows(plan, R.fold_sum), what=f"bnrow_stats c={c} n={n} {family}", family="A sums")
    box = sums_box(ref, mag, R.chain_rows(plan, R.fold_finalize))
    for eps, running in ((1e-3, True), (1e-5, False)):
        dev = run_row_stats_finalize(s, n, c, plan, eps, 0.1, running)
        fn = fwd_fn(s, n, eps, 0.1, running)
        R.check_box(dev, fn, *box, what=f"bnrow_stats_finalize c={c} n={n} {family} eps={eps}", family="A finalize",
                    apart=apart_channels(s, box[0], box[2], n))
        note_invstd(family, dev["invstd"], fn, box[0], box[2], n)


@pytest.mark.parametrize("c", R.ROW_C)
def test_row_stats(c):
    for n, family in families([n for cc, n in R.ROW["cases"] if cc == c]):
        check_row_stats(c, n, family)


BWD_REDUCE_FORMS = ((0, False), (1, True), (1, False), (2, False))   # (act, mask from y)


def bwd_reduce_ref(s, act, use_y):
    z, _ = R.ref_z(s.x, s.scale, s.shift)
    g, gerr = R.ref_g(s.dy, act, z=z, y=s.y if use_y else None)
    return R.ref_bwd_sums(g, gerr, s.x)


def dy_operand(s, n, c, ld):
    """dy as a channel slice of a wider tensor whose other channels are NaN: a finite result shows they were not read"""
    buf, sl, _ = R.wide(n, c, ld, s.dy.dtype, DEV)
    sl.copy_(s.dy)
    return buf, sl


def run_row_bwd_reduce(s, n, c, plan, act, use_y, ld, copy):
    dbuf, dy = dy_operand(s, n, c, ld)
    mask = (p(s.y) if use_y else None, p(s.scale) if act and not use_y else None, p(s.shift) if act and not use_y else None)

    def run(ws, nb):
        buf, st = fvec(2 * c)
        cbuf, cp = fvec(2 * c)
        if ld == c:
            ok("s2d_bnrow_bwd_reduce_bf16", p(dy), p(s.x), *mask, act, n, c, p(st), p(cp) if copy else None, ws, nb, stream())
        else:
            ok("s2d_bnrow_bwd_reduce_ld_bf16", p(dy), ld, p(s.x), *mask, act, n, c, p(st), p(cp) if copy else None, ws, nb, stream())
        torch.cuda.synchronize()
        fvec_ok(buf, 2 * c, "bnrow_bwd_reduce sums")
        fvec_ok(cbuf, 2 * c if copy else 0, "bnrow_bwd_reduce sums_copy")
        if copy:
            R.check_bits(cp, st, "sums_copy against sums", "index")
        return (st.clone(),)
    return with_ws(plan.ws_bytes, run)[0]


def run_row_bwd_reduce_finalize(s, n, c, plan, act, use_y, ld):
    dbuf, dy = dy_operand(s, n, c, ld)
    mask = (p(s.y) if use_y else None, p(s.scale) if act and not use_y else None, p(s.shift) if act and not use_y else None)

    def run(ws, nb):
        out = ChanOut(BWD, c)
        tail = (act, n, c, p(s.gamma), p(s.mean), p(s.invstd), *[out.ptr(k) for k in BWD], ws, nb, stream())
        if ld == c:
            ok("s2d_bnrow_bwd_reduce_finalize_bf16", p(dy), p(s.x), *mask, *tail)
        else:
            ok("s2d_bnrow_bwd_reduce_finalize_ld_bf16", p(dy), ld, p(s.x), *mask, *tail)
        return chan_tuple(out.result("bnrow_bwd_reduce_finalize"))
    return dict(zip(sorted(BWD), with_ws(plan.ws_bytes, run)))


def check_row_bwd_reduce(c, n, family, forms=BWD_REDUCE_FORMS, lds=None):
    s = row_case(c, n, family)
    plan = row_plan_checked(n, c)
    for act, use_y in forms:
        ref, mag, act_sum = bwd_reduce_ref(s, act, use_y)
        for ld in lds or R.row_lds(c):
            what = f"c={c} n={n} {family} act={act} y={use_y} dy_ld={ld}"
            for copy in (False, True):   # sums_copy null and non-null, at every row stride and so through both entries
                st = run_row_bwd_reduce(s, n, c, plan, act, use_y, ld, copy)
                R.check_sums(st, ref, mag, R.chain_rows(plan, R.fold_sum), act_sum, what=f"bnrow_bwd_reduce {what} sums_copy={copy}", family="A bwd sums")
            dev = run_row_bwd_reduce_finalize(s, n, c, plan, act, use_y, ld)
            R.check_box(dev, bwd_fn(s, n), *sums_box(ref, mag, R.chain_rows(plan, R.fold_finalize), act_sum),
                        what="bnrow_bwd_reduce_finalize " + what, family="A bwd finalize")


@pytest.mark.parametrize("c", R.ROW_C)
def test_row_bwd_reduce(c):
    for n, family in families([n for cc, n in R.ROW["cases"] if cc == c]):
        check_row_bwd_reduce(c, n, family)


def run_row_apply(s, n, c, res, act, ld):
    buf, y, off = R.wide(n, c, ld, BF, DEV)
    if ld == c:
        ok("s2d_bnrow_apply_bf16", p(s.x), p(s.scale), p(s.shift), p(res), act, n, c, p(y), stream())
    else:
        ok("s2d_bnrow_apply_ld_bf16", p(s.x), p(s.scale), p(s.shift), p(res), act, n, c, p(y), ld, stream())
    torch.cuda.synchronize()
    R.assert_slice_written(buf, off, c, f"bnrow_apply y_ld={ld}")
    return y


@pytest.mark.parametrize("c", R.ROW_C)
def test_row_apply(c):
    for n, family in families([n for cc, n in R.ROW["cases"] if cc == c]):
        s = row_case(c, n, family)
        assert R.row_launch(n, c).trips == 1
        for with_res in (False, True):
            for act in (0, 1, 2):
                ref, mag, term = R.ref_apply(s.x, s.scale, s.shift, s.res if with_res else None, act)
                for ld in R.row_lds(c):
                    y = run_row_apply(s, n, c, s.res if with_res else None, act, ld)
                    R.check_elementwise(y, ref, mag, term, what=f"bnrow_apply c={c} n={n} {family} res={with_res} act={act} y_ld={ld}",
                                        family="A apply gelu" if act == 2 else "A apply")


BWD_APPLY_FORMS = [(act, use_y, dres) for act, use_y in BWD_REDUCE_FORMS for dres in (False, True)]   # the dispatcher's eight


def run_row_bwd_apply(s, n, c, act, use_y, with_dres, ld):
    dbuf, dy = dy_operand(s, n, c, ld)
    xbuf, dx = R.poisoned(n, c, dtype=BF, device=DEV)
    rbuf, dres = R.poisoned(n, c, dtype=BF, device=DEV)
    mask = (p(s.y) if use_y else None, p(s.scale) if act and not use_y else None, p(s.shift) if act and not use_y else None)
    tail = (*mask, act, p(s.a), p(s.b), p(s.d), n, c, p(dx), p(dres) if with_dres else None, stream())
    if ld == c:
        ok("s2d_bnrow_bwd_apply_bf16", p(dy), p(s.x), *tail)
    else:
        ok("s2d_bnrow_bwd_apply_ld_bf16", p(dy), ld, p(s.x), *tail)
    torch.cuda.synchronize()
    R.assert_written(xbuf, "bnrow_bwd_apply dx")
    if with_dres:
        R.assert_written(rbuf, "bnrow_bwd_apply dres")
    else:
        R.assert_untouched(rbuf, "bnrow_bwd_apply dres (not requested)")
    return dx, dres if with_dres else None


def check_row_bwd_apply(s, n, c, act, use_y, with_dres, ld, what):
    dx, dres = run_row_bwd_apply(s, n, c, act, use_y, with_dres, ld)
    for r0 in range(0, n, 16384):
        sl = slice(r0, min(r0 + 16384, n))
        z, _ = R.ref_z(s.x[sl], s.scale, s.shift)
        g, gerr = R.ref_g(s.dy[sl], act, z=z, y=s.y[sl] if use_y else None)
        ref, mag, term = R.ref_bwd_apply(g, gerr, s.x[sl], s.a, s.b, s.d)
        R.check_elementwise(dx[sl], ref, mag, term, what=f"bnrow_bwd_apply dx {what} rows from {r0}", family="A bwd apply gelu" if act == 2 else "A bwd apply")
        if dres is not None and act == 2:
            R.check_elementwise(dres[sl], g, g.abs(), gerr, what=f"bnrow_bwd_apply dres {what} rows from {r0}", family="A bwd apply gelu")
        elif dres is not None:
            R.check_bits(dres[sl], g.to(BF), f"bnrow_bwd_apply dres {what} rows from {r0}")   # g is dy or zero: exact in bf16


@pytest.mark.parametrize("c", R.ROW_C)
def test_row_bwd_apply(c):
    for n, family in families([n for cc, n in R.ROW["cases"] if cc == c]):
        s = row_case(c, n, family)
        for act, use_y, with_dres in BWD_APPLY_FORMS:
            for ld in R.row_lds(c):
                check_row_bwd_apply(s, n, c, act, use_y, with_dres, ld, f"c={c} n={n} {family} act={act} y={use_y} dres={with_dres} dy_ld={ld}")


@pytest.mark.parametrize("c,n", R.ROW["reduce_cap"])
def test_row_reduce_cap(c, n):
    """the 2048-workgroup cap of row_plan_bf16: trailing workgroups are empty and write zero partials that the fold kernels take in"""
    plan = R.row_plan_bf16(n, c)
    assert plan.nblocks == R.ROW_REDUCE_CAP and plan.empty > 0 and R.row_plan_bf16(n - 1 if c == 1024 else 2048 * 32, c).empty == 0
    if (c, n) == (1024, 32769):
        assert (plan.rows_per_block, plan.empty) == (17, 120)
    check_row_stats(c, n, "benign")
    check_row_bwd_reduce(c, n, "benign", forms=((1, False),), lds=(c,))


def test_row_apply_cap():
    """the 16384-workgroup cap of row_launch: the second trip of the apply and backward-apply loops (tensors of 256 MiB)"""
    c, n = R.ROW["apply_cap"]
    assert R.row_launch(n, c).trips == 2 and R.row_launch(n - 1, c).trips == 1
    s = params(c, "benign", 5)
    g = gen(6)
    s.x = torch.empty(n, c, dtype=BF, device=DEV).normal_(0.3, 2.0, generator=g)
    s.res = torch.empty(n, c, dtype=BF, device=DEV).normal_(0.0, 1.0, generator=g)
    s.dy, s.y = s.res, None
    s.x[:, 1], s.x[:, 3] = 1.0, 0.30078125
    for r0 in range(0, n, 16384):
        assert R.make_unambiguous(s.x[r0:r0 + 16384], s.scale, s.shift) == 0
    y = run_row_apply(s, n, c, s.res, 1, c)
    for r0 in range(0, n, 16384):
        sl = slice(r0, min(r0 + 16384, n))
        ref, mag, term = R.ref_apply(s.x[sl], s.scale, s.shift, s.res[sl], 1)
        R.check_elementwise(y[sl], ref, mag, term, what=f"bnrow_apply at the launch cap, rows from {r0}", family="A apply")
    del y
    check_row_bwd_apply(s, n, c, 1, False, True, c, "at the launch cap")


@pytest.mark.parametrize("what,c,n,ld_extra,short,relu,code", R.ROW["refused"], ids=[r[0] for r in R.ROW["refused"]])
def test_row_refused(what, c, n, ld_extra, short, relu, code):
    """error returns that reach no launch: the documented code, every output still at its poison"""
    cc, rows_ = 1040, 48
    x = torch.ones(rows_, cc, dtype=BF, device=DEV)
    v = torch.ones(cc, device=DEV)
    ybuf, y = R.poisoned(rows_, 3 * cc, dtype=BF, device=DEV)
    dbuf, dx = R.poisoned(rows_, cc, dtype=BF, device=DEV)
    sbuf, st = fvec(2 * cc + 2)
    out = ChanOut(FWD + BWD, cc)
    ws_bytes = max(call("s2d_bnrow_workspace_bytes", max(n, 1), c if c % 8 == 0 and c <= 1024 else 64) - short, 0)
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=DEV)
    ld = c + ld_extra
    if c % 8 or c > 1024:
        assert call("s2d_bnrow_workspace_bytes", n, c) == 0
    codes = {}
    if relu <= 2 and not ld_extra:
        codes["stats"] = call("s2d_bnrow_stats_bf16", p(x), n, c, p(st), 1, p(ws), ws_bytes, stream())
        codes["stats_finalize"] = call("s2d_bnrow_stats_finalize_bf16", p(x), n, c, p(v), p(v), 1e-3, 0.1, out.ptr("mean"), out.ptr("invstd"),
                                       out.ptr("scale"), out.ptr("shift"), None, None, None, p(ws), ws_bytes, stream())
    codes["bwd_reduce"] = call("s2d_bnrow_bwd_reduce_ld_bf16", p(x), ld, p(x), None, p(v), p(v), relu, n, c, p(st), None, p(ws), ws_bytes, stream())
    codes["bwd_reduce_finalize"] = call("s2d_bnrow_bwd_reduce_finalize_ld_bf16", p(x), ld, p(x), None, p(v), p(v), relu, n, c, p(v), p(v), p(v),
                                        *[out.ptr(k) for k in BWD], p(ws), ws_bytes, stream())
    if not short:
        codes["apply"] = call("s2d_bnrow_apply_ld_bf16", p(x), p(v), p(v), None, relu, n, c, p(y), ld, stream())
        codes["bwd_apply"] = call("s2d_bnrow_bwd_apply_ld_bf16", p(x), ld, p(x), None, p(v), p(v), relu, p(v), p(v), p(v), n, c, p(dx), None, stream())
    torch.cuda.synchronize()
    assert all(rc == code for rc in codes.values()), (what, code, codes)
    for buf, name in ((ybuf, "y"), (dbuf, "dx"), (sbuf, "sums")) + tuple((b, k) for k, (b, _) in out.bufs.items()):
        R.assert_untouched(buf, f"{what}: {name}")


@pytest.mark.parametrize("c,n", R.ROW["fused_vs_split"])
def test_row_fused_against_split(c, n):
    """E. the fused bf16 entries and the split (SyncBN) route - stats_bf16 -> bn1d_finalize_fwd_f32, bwd_reduce_bf16 ->
    bn1d_finalize_bwd_f32 with a count word - both meet the same reference"""
    for family in ("benign", "offset"):
        s = row_case(c, n, family)
        plan = row_plan_checked(n, c)
        ref, mag = R.ref_sums(s.x)
        check_row_stats(c, n, family)
        st = torch.cat([run_row_stats(s, n, c, plan, 0), torch.tensor([float(n)], device=DEV)])
        out = ChanOut(FWD + RUN, c, {"running_mean": s.rm, "running_var": s.rv})
        bt = torch.zeros(1, dtype=torch.int64, device=DEV)
        ok("s2d_bn1d_finalize_fwd_f32", p(st), p(st[2 * c:]), p(s.gamma), p(s.beta), 1e-3, 0.1, c, *[out.ptr(k) for k in FWD + RUN], p(bt), stream())
        dev = out.result("bn1d_finalize_fwd")
        assert int(bt) == 1
        fn = fwd_fn(s, n, 1e-3, 0.1, True)
        box = sums_box(ref, mag, R.chain_rows(plan, R.fold_sum))
        R.check_box(dev, fn, *box, what=f"split forward c={c} n={n} {family}", family="E split", apart=apart_channels(s, box[0], box[2], n))
        note_invstd(family, dev["invstd"], fn, box[0], box[2], n)
        for act, use_y in BWD_REDUCE_FORMS:
            bref, bmag, act_sum = bwd_reduce_ref(s, act, use_y)
            fused = run_row_bwd_reduce_finalize(s, n, c, plan, act, use_y, c)
            R.check_box(fused, bwd_fn(s, n), *sums_box(bref, bmag, R.chain_rows(plan, R.fold_finalize), act_sum), what="fused backward", family="E fused")
            sums = run_row_bwd_reduce(s, n, c, plan, act, use_y, c, True)
            out = ChanOut(BWD, c)
            ok("s2d_bn1d_finalize_bwd_f32", p(sums), p(sums), p(st[2 * c:]), p(s.gamma), p(s.mean), p(s.invstd), c, *[out.ptr(k) for k in BWD], stream())
            R.check_box(out.result("bn1d_finalize_bwd"), bwd_fn(s, n), *sums_box(bref, bmag, R.chain_rows(plan, R.fold_sum), act_sum),
                        what=f"split backward c={c} n={n} {family} act={act}", family="E split")


# ======== B. row-major fp32 ==============================================================================================================
def red_plan_checked(n, c):
    plan = R.red_plan(n, c)
    assert call("s2d_bn1d_workspace_bytes", n, c) == plan.ws_bytes, ("the mirrored fp32 reduce plan is not the one taken", n, c, plan)
    return plan


def bn1d_forward(s, n, c, plan, family):
    ref, mag = R.ref_sums(s.x)

    def run(ws, nb):
        buf, st = fvec(2 * c + 1)
        ok("s2d_bn1d_stats_f32", p(s.x), n, c, p(st), ws, nb, stream())
        torch.cuda.synchronize()
        fvec_ok(buf, 2 * c, "bn1d_stats")
        return (st[:2 * c].clone(),)
    (st,) = with_ws(plan.ws_bytes, run)
    R.check_sums(st, ref, mag, R.chain_rows(plan, R.fold_sum), what=f"bn1d_stats c={c} n={n} {family}", family="B sums")
    for eps, running in ((1e-3, True), (1e-5, False)):
        fn = fwd_fn(s, n, eps, 0.1, running)
        dev = run_row_stats_finalize(s, n, c, plan, eps, 0.1, running, name="s2d_bn1d_stats_finalize_f32")
        box = sums_box(ref, mag, R.chain_rows(plan, R.fold_finalize))
        R.check_box(dev, fn, *box, what=f"bn1d_stats_finalize c={c} n={n} {family} eps={eps}", family="B finalize",
                    apart=apart_channels(s, box[0], box[2], n))
        note_invstd(family, dev["invstd"], fn, box[0], box[2], n)
        # the split route: the sums above and a count word
        stc = torch.cat([st, torch.tensor([float(n)], device=DEV)])
        names = FWD + (RUN if running else ())
        out = ChanOut(names, c, {"running_mean": s.rm, "running_var": s.rv} if running else None)
        ok("s2d_bn1d_finalize_fwd_f32", p(stc), p(stc[2 * c:]), p(s.gamma), p(s.beta), eps, 0.1, c, *[out.ptr(k) for k in FWD + RUN], None, stream())
        R.check_box(out.result("bn1d_finalize_fwd"), fn, *sums_box(ref, mag, R.chain_rows(plan, R.fold_sum)),
                    what=f"bn1d split forward c={c} n={n} {family} eps={eps}", family="B finalize", apart=apart_channels(s, box[0], box[2], n))


def bn1d_apply(s, n, c, family):
    for with_res in (False, True):
        for relu in (0, 1):
            buf, y = R.poisoned(n, c, dtype=F32, device=DEV)
            ok("s2d_bn1d_apply_f32", p(s.x), p(s.scale), p(s.shift), p(s.res) if with_res else None, relu, n, c, p(y), stream())
            torch.cuda.synchronize()
            R.assert_written(buf, "bn1d_apply y")
            ref, mag, _ = R.ref_apply(s.x, s.scale, s.shift, s.res if with_res else None, relu)
            R.check_elementwise(y, ref, mag, what=f"bn1d_apply c={c} n={n} {family} res={with_res} relu={relu}", family="B apply")
    buf, dx = R.poisoned(n, c, dtype=F32, device=DEV)
    ok("s2d_bn1d_bwd_apply_f32", p(s.dy), p(s.x), p(s.a), p(s.b), p(s.d), n, c, p(dx), stream())
    torch.cuda.synchronize()
    R.assert_written(buf, "bn1d_bwd_apply dx")
    ref, mag, _ = R.ref_bwd_apply(s.dy.double(), torch.zeros_like(ref), s.x, s.a, s.b, s.d)
    R.check_elementwise(dx, ref, mag, what=f"bn1d_bwd_apply c={c} n={n} {family}", family="B bwd apply")


def bn1d_backward(s, n, c, plan, family):
    for relu in (0, 1):
        g, gerr = R.ref_g(s.dy, relu, y=s.y)
        ref, mag, _ = R.ref_bwd_sums(g, gerr, s.x)
        for with_g in (False, True):
            def run(ws, nb):
                buf, st = fvec(2 * c)
                gbuf, g_out = R.poisoned(n, c, dtype=F32, device=DEV)
                ok("s2d_bn1d_bwd_reduce_f32", p(s.dy), p(s.y) if relu else None, p(s.x), relu, n, c, p(g_out) if with_g else None, p(st), ws, nb, stream())
                torch.cuda.synchronize()
                fvec_ok(buf, 2 * c, "bn1d_bwd_reduce sums")
                if with_g:
                    R.assert_written(gbuf, "bn1d_bwd_reduce g_out")
                    R.check_bits(g_out, g.float(), "g_out against the masked dy")
                else:
                    R.assert_untouched(gbuf, "g_out (not requested)")
                return (st.clone(),)
            (st,) = with_ws(plan.ws_bytes, run)
            what = f"c={c} n={n} {family} relu={relu} g_out={with_g}"
            R.check_sums(st, ref, mag, R.chain_rows(plan, R.fold_sum), what="bn1d_bwd_reduce " + what, family="B bwd sums")

            def run_fused(ws, nb):
                out = ChanOut(BWD, c)
                gbuf, g_out = R.poisoned(n, c, dtype=F32, device=DEV)
                ok("s2d_bn1d_bwd_reduce_finalize_f32", p(s.dy), p(s.y) if relu else None, p(s.x), relu, n, c, p(s.gamma), p(s.mean), p(s.invstd),
                   p(g_out) if with_g else None, *[out.ptr(k) for k in BWD], ws, nb, stream())
                res = out.result("bn1d_bwd_reduce_finalize")
                if with_g:
                    R.check_bits(g_out, g.float(), "g_out against the masked dy")
                return chan_tuple(res)
            dev = dict(zip(sorted(BWD), with_ws(plan.ws_bytes, run_fused)))
            R.check_box(dev, bwd_fn(s, n), *sums_box(ref, mag, R.chain_rows(plan, R.fold_finalize)), what="bn1d_bwd_reduce_finalize " + what, family="B bwd finalize")
        # the split backward as a 3-rank SyncBN all-reduce hands it over: global sums = 3 x local, count = 3 n.  dgamma / dbeta follow the
        # local sums, a / b / d the global ones; 3 * s is one more fp32 rounding (2^-24 |3 s|) on top of three times the local bound
        glob = st * 3.0
        cnt = torch.tensor([float(3 * n)], device=DEV)
        out = ChanOut(BWD, c)
        ok("s2d_bn1d_finalize_bwd_f32", p(st), p(glob), p(cnt), p(s.gamma), p(s.mean), p(s.invstd), c, *[out.ptr(k) for k in BWD], stream())
        dev = out.result("bn1d_finalize_bwd")
        chain = R.chain_rows(plan, R.fold_sum)
        R.check_box({k: dev[k] for k in ("dgamma", "dbeta")}, lambda a, b: R.bwd_finalize_local(a, b, s.mean, s.invstd), *sums_box(ref, mag, chain),
                    what=f"bn1d split backward (local) c={c} n={n} relu={relu}", family="B bwd finalize")
        R.check_box({k: dev[k] for k in ("a", "b", "d")}, lambda a, b: R.bwd_finalize_global(a, b, 3 * n, s.gamma, s.mean, s.invstd),
                    *sums_box(3 * ref, 3 * mag + 3 * ref.abs() / chain, chain), what=f"bn1d split backward (global) c={c} n={n} relu={relu}",
                    family="B bwd finalize")


@pytest.mark.parametrize("c", R.BN1D_C)
def test_bn1d(c):
    for n, family in families([n for cc, n in R.BN1D["cases"] if cc == c]):
        s = row_case(c, n, family, F32)
        plan = red_plan_checked(n, c)
        bn1d_forward(s, n, c, plan, family)
        bn1d_apply(s, n, c, family)
        bn1d_backward(s, n, c, plan, family)


def test_bn1d_reduce_cap():
    c, n = R.BN1D["reduce_cap"]
    plan = red_plan_checked(n, c)
    assert plan.nblocks == R.RED_CAP and plan.empty > 0 and R.red_plan(n - 1, c).empty == 0
    s = row_case(c, n, "benign", F32)
    bn1d_forward(s, n, c, plan, "benign")
    bn1d_backward(s, n, c, plan, "benign")


def test_bn1d_apply_cap():
    c, n = R.BN1D["apply_cap"]
    assert R.bn_apply_trips(n, c) == 2 and R.bn_apply_trips(n - 1, c) == 1
    bn1d_apply(row_case(c, n, "benign", F32), n, c, "benign")


def test_bn1d_no_rows():
    """n = 0: the sums are zeroed, apply and backward apply are no-ops"""
    c = 16
    v = torch.ones(c, device=DEV)
    for name in ("s2d_bn1d_stats_f32", "s2d_bn1d_bwd_reduce_f32"):
        buf, st = fvec(2 * c + 1)
        if name == "s2d_bn1d_stats_f32":
            ok(name, None, 0, c, p(st), None, 0, stream())
        else:
            ok(name, None, None, None, 1, 0, c, None, p(st), None, 0, stream())
        torch.cuda.synchronize()
        fvec_ok(buf, 2 * c, name)
        assert bool((st[:2 * c] == 0).all())
    buf, y = R.poisoned(4, c, dtype=F32, device=DEV)
    ok("s2d_bn1d_apply_f32", p(y), p(v), p(v), None, 1, 0, c, p(y), stream())
    ok("s2d_bn1d_bwd_apply_f32", p(y), p(y), p(v), p(v), p(v), 0, c, p(y), stream())
    torch.cuda.synchronize()
    R.assert_untouched(buf, "bn1d apply with n = 0")


# ======== C. channel-major =============================================================================================================
def cm_case(batch, c, pos, seed=0, family="benign"):
    g = gen(batch * 1000 + c * 10 + pos % 997 + seed)
    s = types.SimpleNamespace()
    rn = lambda: torch.randn(c, device=DEV, generator=g)
    s.scale, s.shift, s.a, s.b, s.d = rn() * 0.5 + 1.0, rn() * 0.5, rn(), rn() * 0.1, rn() * 0.1
    s.x = torch.randn(batch, c, pos, device=DEV, generator=g) * 2.0 + 0.3
    if family == "offset":
        s.x, s.shift = (s.x - 0.3) * 0.25 + 8.0, s.shift - 8.0 * s.scale
    if c > 2:
        s.x[:, 1], s.scale[1], s.shift[1] = 1.0, 1.0, -1.0       # exact zeros of z
        s.scale[2] = s.a[2] = 0.0
    s.dy = torch.randn(batch, c, pos, device=DEV, generator=g)
    s.y = torch.randn(batch, c, pos, device=DEV, generator=g).clamp_min(0.0)
    s.v = lambda t: t.view(1, c, 1)
    assert R.make_unambiguous(s.x, s.v(s.scale), s.v(s.shift)) == 0
    return s


def cm_sums(name, args, c, plan, what):
    def run(ws, nb):
        buf, st = fvec(2 * c)
        ok(name, *args(p(st), ws, nb))
        torch.cuda.synchronize()
        fvec_ok(buf, 2 * c, what)
        return (st.clone(),)
    return with_ws(plan.ws_bytes, run)[0]


def cm_elementwise(name, args, shape, dtype, what):
    buf, out = R.poisoned(shape[0], *shape[1:], dtype=dtype, device=DEV)
    ok(name, *args(p(out)))
    torch.cuda.synchronize()
    R.assert_written(buf, what)
    return out


def check_cm(batch, c, pos, family="benign"):
    s = cm_case(batch, c, pos, family=family)
    plan = R.cm_plan(batch, c, pos)
    assert call("s2d_bncm_workspace_bytes", batch, c, pos) == plan.ws_bytes, ("the mirrored channel-major plan is not the one taken", plan)
    chain = R.chain_cm(batch, plan)
    dims, names, what = (0, 2), "sample, channel, position", f"batch={batch} c={c} positions={pos} {family}"
    sc, sh = s.v(s.scale), s.v(s.shift)
    ref, mag = R.ref_sums(s.x, dims)
    st = cm_sums("s2d_bncm_stats_f32", lambda o, ws, nb: (p(s.x), batch, c, pos, o, ws, nb, stream()), c, plan, "bncm_stats")
    R.check_sums(st, ref, mag, chain, what="bncm_stats " + what, family="C sums")
    z, _ = R.ref_z(s.x, sc, sh)
    gx, _ = R.ref_g(s.dy, 1, z=z)
    gy, _ = R.ref_g(s.dy, 1, y=s.y)
    zero = torch.zeros_like(gx)
    for relu, g in ((0, s.dy.double()), (1, gy)):
        ref, mag, _ = R.ref_bwd_sums(g, zero, s.x, dims)
        st = cm_sums("s2d_bncm_bwd_reduce_f32", lambda o, ws, nb: (p(s.dy), p(s.y) if relu else None, p(s.x), relu, batch, c, pos, o, ws, nb, stream()),
                     c, plan, "bncm_bwd_reduce")
        R.check_sums(st, ref, mag, chain, what=f"bncm_bwd_reduce relu={relu} " + what, family="C sums")
        dx = cm_elementwise("s2d_bncm_bwd_apply_f32", lambda o: (p(s.dy), p(s.y) if relu else None, p(s.x), p(s.a), p(s.b), p(s.d), relu, batch, c, pos, o,
                                                                stream()), s.x.shape, F32, "bncm_bwd_apply")
        r, m, _ = R.ref_bwd_apply(g, zero, s.x, s.v(s.a), s.v(s.b), s.v(s.d))
        R.check_elementwise(dx, r, m, what=f"bncm_bwd_apply relu={relu} " + what, family="C apply", names=names)
    ref, mag, _ = R.ref_bwd_sums(gx, zero, s.x, dims)
    st = cm_sums("s2d_bncm_bwd_reduce_x_f32", lambda o, ws, nb: (p(s.dy), p(s.x), p(s.scale), p(s.shift), batch, c, pos, o, ws, nb, stream()),
                 c, plan, "bncm_bwd_reduce_x")
    R.check_sums(st, ref, mag, chain, what="bncm_bwd_reduce_x " + what, family="C sums")
    dx = cm_elementwise("s2d_bncm_bwd_apply_x_f32", lambda o: (p(s.dy), p(s.x), p(s.scale), p(s.shift), p(s.a), p(s.b), p(s.d), batch, c, pos, o, stream()),
                        s.x.shape, F32, "bncm_bwd_apply_x")
    r, m, _ = R.ref_bwd_apply(gx, zero, s.x, s.v(s.a), s.v(s.b), s.v(s.d))
    R.check_elementwise(dx, r, m, what="bncm_bwd_apply_x " + what, family="C apply", names=names)
    for relu in (0, 1):
        y = cm_elementwise("s2d_bncm_apply_f32", lambda o: (p(s.x), p(s.scale), p(s.shift), relu, batch, c, pos, o, stream()), s.x.shape, F32, "bncm_apply")
        r, m, _ = R.ref_apply(s.x, sc, sh, None, relu)
        R.check_elementwise(y, r, m, what=f"bncm_apply relu={relu} " + what, family="C apply", names=names)


@pytest.mark.parametrize("batch,c,pos", R.CM["cases"] + [R.CM["chunks_by_channels"], R.CM["apply_cap"]])
def test_cm(batch, c, pos):
    if (batch, c, pos) == R.CM["chunks_by_channels"]:
        assert R.cm_plan(batch, c, pos).chunks == R.ceil_div(2048, c) < R.ceil_div(pos // 4, 1024)
    if (batch, c, pos) == R.CM["apply_cap"]:
        assert R.cm_apply_trips(pos) == 2 and R.cm_apply_trips(pos - 4) == 1
    if pos == 4100:
        assert R.cm_plan(batch, c, pos).chunks == 2 and pos // 4 == 1025
        check_cm(batch, c, pos, "offset")
    check_cm(batch, c, pos)


@pytest.mark.parametrize("batch,c,pos,family", [(2, 16, 4100, "benign"), (2, 16, 4100, "offset"), (3, 3, 1020, "benign")])
def test_cm_typed(batch, c, pos, family):
    """the bf16-storage forms: the three supported (dy, x, dx) storage combinations against float64 on the stored operands (a bf16 dx
    to the half-ulp criterion); every other combination is refused with the outputs untouched"""
    s = cm_case(batch, c, pos, seed=1, family=family)
    plan = R.cm_plan(batch, c, pos)
    assert call("s2d_bncm_workspace_bytes", batch, c, pos) == plan.ws_bytes, ("the mirrored channel-major plan is not the one taken", plan)
    chain = R.chain_cm(batch, plan)
    names = "sample, channel, position"
    for dy16, x16, dx16 in [(a, b, d) for a in (0, 1) for b in (0, 1) for d in (0, 1)]:
        x = s.x.to(BF) if x16 else s.x.clone()
        dy = s.dy.to(BF) if dy16 else s.dy
        assert R.make_unambiguous(x, s.v(s.scale), s.v(s.shift)) == 0
        supported = (dy16, x16, dx16) in R.CM["typed"]
        buf, dx = R.poisoned(batch, c, pos, dtype=BF if dx16 else F32, device=DEV)
        rc = call("s2d_bncm_bwd_apply_x_typed", p(dy), dy16, p(x), x16, p(s.scale), p(s.shift), p(s.a), p(s.b), p(s.d), batch, c, pos, p(dx), dx16, stream())
        torch.cuda.synchronize()
        z, _ = R.ref_z(x, s.v(s.scale), s.v(s.shift))
        g, _ = R.ref_g(dy, 1, z=z)
        zero = torch.zeros_like(g)
        what = f"dy_bf16={dy16} x_bf16={x16} dx_bf16={dx16} batch={batch} c={c} positions={pos} {family}"
        if supported:
            assert rc == R.S2D_OK, (what, rc)
            R.assert_written(buf, "bncm_bwd_apply_x_typed")
            r, m, _ = R.ref_bwd_apply(g, zero, x, s.v(s.a), s.v(s.b), s.v(s.d))
            R.check_elementwise(dx, r, m, what="bncm_bwd_apply_x_typed " + what, family="C typed", names=names)
        else:
            assert rc == R.S2D_ERR_UNSUPPORTED, (what, rc)
            R.assert_untouched(buf, "bncm_bwd_apply_x_typed " + what)
        if dx16:
            continue
        sbuf, st = fvec(2 * c)
        if (dy16, x16) in [(a, b) for a, b, _ in R.CM["typed"]]:
            st = cm_sums("s2d_bncm_bwd_reduce_x_typed", lambda o, ws, nb: (p(dy), dy16, p(x), x16, p(s.scale), p(s.shift), batch, c, pos, o, ws, nb, stream()),
                         c, plan, "bncm_bwd_reduce_x_typed")
            ref, mag, _ = R.ref_bwd_sums(g, zero, x, (0, 2))
            R.check_sums(st, ref, mag, chain, what="bncm_bwd_reduce_x_typed " + what, family="C typed")
        else:
            ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=DEV)
            rc = call("s2d_bncm_bwd_reduce_x_typed", p(dy), dy16, p(x), x16, p(s.scale), p(s.shift), batch, c, pos, p(st), p(ws), plan.ws_bytes, stream())
            torch.cuda.synchronize()
            assert rc == R.S2D_ERR_UNSUPPORTED, (what, rc)
            R.assert_untouched(sbuf, "bncm_bwd_reduce_x_typed " + what)


def test_cm_rejects_positions_not_a_multiple_of_four():
    pos, c = R.CM["rejected_positions"], 4
    assert call("s2d_bncm_workspace_bytes", 1, c, pos) == 0
    x = torch.ones(1, c, 8, device=DEV)
    v = torch.ones(c, device=DEV)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    sbuf, st = fvec(2 * c)
    ybuf, y = R.poisoned(1, c, 8, dtype=F32, device=DEV)
    codes = [call("s2d_bncm_stats_f32", p(x), 1, c, pos, p(st), p(ws), 4096, stream()),
             call("s2d_bncm_bwd_reduce_x_f32", p(x), p(x), p(v), p(v), 1, c, pos, p(st), p(ws), 4096, stream()),
             call("s2d_bncm_bwd_reduce_x_typed", p(x), 0, p(x), 0, p(v), p(v), 1, c, pos, p(st), p(ws), 4096, stream()),
             call("s2d_bncm_bwd_reduce_f32", p(x), p(x), p(x), 1, 1, c, pos, p(st), p(ws), 4096, stream())]
    assert codes == [R.S2D_ERR_UNSUPPORTED] * 4, codes
    codes = [call("s2d_bncm_apply_f32", p(x), p(v), p(v), 1, 1, c, pos, p(y), stream()),
             call("s2d_bncm_bwd_apply_x_f32", p(x), p(x), p(v), p(v), p(v), p(v), p(v), 1, c, pos, p(y), stream()),
             call("s2d_bncm_bwd_apply_f32", p(x), p(x), p(x), p(v), p(v), p(v), 1, 1, c, pos, p(y), stream()),
             call("s2d_bncm_bwd_apply_x_typed", p(x), 0, p(x), 0, p(v), p(v), p(v), p(v), p(v), 1, c, pos, p(y), 0, stream())]
    assert codes == [R.S2D_ERR_INVALID_ARG] * 4, codes
    torch.cuda.synchronize()
    R.assert_untouched(sbuf, "sums")
    R.assert_untouched(ybuf, "y")


# ======== D. partial-list finalizers =====================================================================================================
@functools.lru_cache(maxsize=2)
def partial_rows(nblocks, c, family, backward):
    """[nblocks, 2c] rows whose column sums are a plausible (sum x, sum x^2) resp. (sum g, sum g x) of 64 rows per tile"""
    g = gen(nblocks * 7 + c + backward)
    m = torch.randn(nblocks, c, device=DEV, generator=g)
    v = torch.randn(nblocks, c, device=DEV, generator=g)
    if backward:
        return torch.cat([64 * 0.1 * m, 64 * 0.2 * v], 1).contiguous()
    mean, var = (0.3 + 0.25 * m, 4.0 * (1 + 0.1 * v).abs()) if family == "benign" else (8.0 + 0.06 * m, 0.25 * (1 + 0.1 * v).abs())
    part = torch.cat([64 * mean, 64 * (var + mean * mean)], 1).contiguous()
    # the constant channels: every tile holds (64 v, 64 v^2), both exact in fp32, so the float64 variance of the list is exactly 0 and the
    # finalize kernel clamps.  v = 1.0 sums exactly in fp32 at every list length; 64 v^2 of v = 77/256 needs more than 24 bits from 2^11 rows on
    for ch, const in PARTIAL_CONSTANTS:
        part[:, ch], part[:, c + ch] = 64 * const, 64 * const * const
    return part


PARTIAL_CONSTANTS = ((1, 1.0), (3, 0.30078125))


@pytest.mark.parametrize("nblocks,c", R.PARTIALS["cases"])
def test_partials(nblocks, c):
    n = 64 * nblocks
    plan = R.partials_plan(nblocks, c)
    assert plan.prefold == (nblocks > R.PS_LONG and 2 * c <= 256)
    assert call("s2d_bn_partials_sum_workspace_bytes", nblocks, c) == plan.ws_bytes == (R.align_up(R.PS_SLICES * 2 * c * 4, 256) if plan.prefold else 0)
    s = params(c, "benign", nblocks + c)
    for family in ("benign", "offset"):
        part = partial_rows(nblocks, c, family, False)
        ref, mag = part.double().sum(0), part.double().abs().sum(0)
        flat = apart_channels(s, ref[:c], ref[c:], n)
        assert flat.nonzero().flatten().tolist() == sorted([ch for ch, _ in PARTIAL_CONSTANTS] + [2]), "the constant channels and gamma = 0"
        var = ref[c:] / n - (ref[:c] / n) ** 2
        assert all(float(var[ch]) == 0.0 for ch, _ in PARTIAL_CONSTANTS), "the constant channels must have float64 variance exactly 0"
        for eps in (1e-3, 1e-5):
            fn = fwd_fn(s, n, eps, 0.1, True)

            def run(ws, nb, entry_name="s2d_bn_partials_finalize_ws_f32"):
                out = ChanOut(FWD + RUN, c, {"running_mean": s.rm, "running_var": s.rv})
                bt = torch.zeros(1, dtype=torch.int64, device=DEV)
                args = (p(part), nblocks, n, c, p(s.gamma), p(s.beta), eps, 0.1, *[out.ptr(k) for k in FWD + RUN], p(bt))
                ok(entry_name, *args, *((ws, nb) if entry_name.endswith("_ws_f32") else ()), stream())
                res = out.result(entry_name)
                assert int(bt) == 1
                return chan_tuple(res)
            for with_ws_ in ((True, False) if plan.prefold else (True,)):
                box = sums_box(ref, mag, R.chain_partials(nblocks, c, with_ws_, R.fold_finalize))
                a = with_ws(plan.ws_bytes if with_ws_ else 0, run)
                b = with_ws(plan.ws_bytes if with_ws_ else 0, run)
                for t0, t1 in zip(a, b):
                    R.check_bits(t0, t1, "two runs", "channel")
                dev = dict(zip(sorted(FWD + RUN), a))
                R.check_box(dev, fn, *box, what=f"bn_partials_finalize_ws nblocks={nblocks} c={c} {family} eps={eps} ws={with_ws_}",
                            family="D finalize", apart=flat)
                note_invstd("partial lists, " + family, dev["invstd"], fn, box[0], box[2], n)
            one = dict(zip(sorted(FWD + RUN), run(None, 0, "s2d_bn_partials_finalize_f32")))
            R.check_box(one, fn, *sums_box(ref, mag, R.chain_partials(nblocks, c, False, R.fold_finalize)),
                        what=f"bn_partials_finalize nblocks={nblocks} c={c} {family} eps={eps}", family="D finalize", apart=flat)
        # the sums entries on the same list (held at other shapes by test_dense3d_gpu.py)
        for name in ("s2d_bn_partials_sum_ws_f32", "s2d_bn_partials_sum_f32"):
            use = name.endswith("_ws_f32")

            def run_sum(ws, nb):
                buf, st = fvec(2 * c + 2)
                ok(name, p(part), nblocks, n, c, p(st), 1, *((ws, nb) if use else ()), stream())
                torch.cuda.synchronize()
                fvec_ok(buf, 2 * c + 1, name)
                assert float(st[2 * c]) == float(n)
                return (st[:2 * c].clone(),)
            (st,) = with_ws(plan.ws_bytes if use else 0, run_sum)
            R.check_sums(st, ref, mag, R.chain_partials(nblocks, c, use, R.fold_sum), what=f"{name} nblocks={nblocks} c={c}", family="D sums")
    part = partial_rows(nblocks, c, "benign", True)
    ref, mag = part.double().sum(0), part.double().abs().sum(0)
    s.mean, s.invstd = torch.randn(c, device=DEV, generator=gen(c)) * 0.3, torch.rand(c, device=DEV, generator=gen(c + 1)) + 0.5
    for with_ws_ in ((True, False) if plan.prefold else (True,)):
        def run_bwd(ws, nb):
            out = ChanOut(BWD, c)
            ok("s2d_bn_partials_bwd_finalize_ws_f32", p(part), nblocks, n, c, p(s.gamma), p(s.mean), p(s.invstd), *[out.ptr(k) for k in BWD], ws, nb, stream())
            return chan_tuple(out.result("bn_partials_bwd_finalize_ws"))
        a = with_ws(plan.ws_bytes if with_ws_ else 0, run_bwd)
        for t0, t1 in zip(a, with_ws(plan.ws_bytes if with_ws_ else 0, run_bwd)):
            R.check_bits(t0, t1, "two runs", "channel")
        R.check_box(dict(zip(sorted(BWD), a)), bwd_fn(s, n), *sums_box(ref, mag, R.chain_partials(nblocks, c, with_ws_, R.fold_finalize)),
                    what=f"bn_partials_bwd_finalize_ws nblocks={nblocks} c={c} ws={with_ws_}", family="D finalize")


# ======== the yardstick of the GELU term and the report ===================================================================================
def test_gelu_yardstick():
    """E_ACT_MEASURED of bn_pass_ref is what torch's fp32 erf / exp give for gelu_f / gelu_grad_f on this device"""
    MEASURED["e_act"] = R.gelu_yardstick(DEV)
    assert MEASURED["e_act"] <= R.E_ACT_MEASURED, (MEASURED["e_act"], R.E_ACT_MEASURED)
    assert R.E_ACT == R.E_ACT_FACTOR * R.E_ACT_MEASURED and R.E_ACT_FACTOR == 4.0


def _whole_file_selected(request):
    """every test function of this module has at least one item in the session (nothing cut away with -k or a node id)"""
    here = request.node.module
    selected = {it.originalname for it in request.session.items if getattr(it, "module", None) is here}
    return {k for k, v in vars(here).items() if k.startswith("test_") and callable(v)} <= selected


def test_every_entry_of_the_case_tables_was_called(request):
    """the last test of the file: what R.entry recorded is the whole of the case tables (which a host test holds equal to the batch-norm
    names of _lib.SIGNATURES), whenever the whole file was selected; a part of the file can only have called names of the tables"""
    assert R.CALLED <= R.table_entries()
    if _whole_file_selected(request):
        assert R.CALLED == R.table_entries(), ("entries of the case tables that no case reached", sorted(R.table_entries() - R.CALLED))


def report_lines():
    lines = ["family                                                              worst |error| / bound"]
    lines += [f"{k:<68s}{v:.3f}" for k, v in sorted(R.WORST.items())]
    lines += ["", f"E_act measured (torch fp32 erf / exp against float64, z in [-10, 10]): {MEASURED.get('e_act', float('nan')):.3e}; "
              f"recorded {R.E_ACT_MEASURED:.1e}, factor {R.E_ACT_FACTOR:g}, E_ACT = {R.E_ACT:.2e}", ""]
    lines += [f"worst relative invstd error against float64, {k}: {v:.3e}" for k, v in sorted(INVSTD.items())]
    lines += ["", f"entries called: {len(R.CALLED)} of {len(R.table_entries())}"]
    return lines


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    """after the module's last test: with BN_PASS_REPORT=<path> in the environment, what the checkers noted in this process is written there
    (profiles/bn_pass_parity.txt is such a file).  Asserts nothing: every figure in it has passed its check already"""
    yield
    path = os.environ.get("BN_PASS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(report_lines()) + "\n")
