"""TEST INFRASTRUCTURE ONLY - float64 restatements, launch-plan mirrors and checkers for the batch-norm pass kernels of
csrc/features.hip (the s2d_bn1d_*, s2d_bnrow_*, s2d_bncm_* and s2d_bn_partials_* entries).  Imports without a GPU and never
loads the native library: tests/test_bn_passes_gpu.py drives the entries, tests/test_bn_pass_checks_cpu.py shows on the host that
every checker below can fail.

Plan mirrors.  row_plan_bf16 (8 rows per thread), row_launch, red_plan, cm_plan, the 4096-block / 1024-block grid-stride caps of
the fp32 and channel-major apply kernels and the PS_LONG = 1536 / PS_SLICES = 512 prefold are restated in Python.  The GPU tests
take their edge shapes from these and first assert that the *_workspace_bytes query of the library returns
align_up(nblocks * 2c * 4, 256) for the mirrored nblocks: a plan that moved fails there and not silently at another shape.
S2D_ROW_RPT (the library's A/B hook for the rows per thread, read once per process) must not be set: importing this module with
it in the environment raises instead of testing another plan.

Bounds.  Nothing below is fitted to what the kernels return.
  elementwise, the test supplies scale / shift or a / b / d itself, so the float64 value of the formula is exact:
      bf16 output  |out - ref| <= 1/2 ulp_bf16(ref) + 4 ulp_fp32(M)        (one round to nearest + at most three fp32 roundings)
      fp32 output  |out - ref| <= 4 ulp_fp32(M)
      M = |x scale| + |shift| + |res|   resp.   |a g| + |b x| + |d|        (the magnitudes of the terms: cancellation is covered)
      dres / g_out: bit-equal to dy or to zero
  GELU routes add  E_ACT max(1, |z|) |dy or 1|  (times |a| where the factor goes through dx = a g + ...): the accuracy of the device
      library's erff / __expf cannot be derived.  E_ACT_MEASURED = 4.5e-7 is the largest absolute error, against float64 over
      z in [-10, 10], of gelu_f and gelu_grad_f of csrc/s2d_common.h evaluated with torch's own fp32 erf and exp on the MI355X
      (tests/test_bn_passes_gpu.py::test_gelu_yardstick re-measures it and holds it under this constant;
      profiles/bn_pass_parity.txt has the run).  torch's evaluation is a yardstick for fp32 evaluation in general, not the kernel under
      test; because the two libraries' erff / exp differ, E_ACT = E_ACT_FACTOR * E_ACT_MEASURED with E_ACT_FACTOR = 4.
  sums  |s - ref| <= L 2^-24 sum|term| per channel, L = the longest chain of sequential additions the mirrored plan gives one
      accumulator: rows per lane of the reduce kernel + lanes of its LDS fold + ceil(nblocks / 64) + 6 (partial_sum_kernel) or
      ceil(nblocks / 256) + 8 (the one-workgroup-per-channel finalize kernels).  The forward bound of recursive summation; the first
      addition of every chain (0 + x) is exact, which pays for the rounding of the product x * x resp. g * x.
  per-channel finalize outputs: the float64 formula at the four corners of [s0 +- d0] x [s1 +- d1] (d from the sums bound); the
      device value must lie in [min - 8 ulp_fp32(m), max + 8 ulp_fp32(m)], m = the largest intermediate of that output's formula
      (at most seven fp32 operations and one rsqrtf).  Wide where the formula is ill-conditioned, tight where it is not.
  ReLU masks recomputed from x: an element is ambiguous when 0 != |z| < 2^-20 (|x scale| + |shift|) in float64.  make_unambiguous()
      nudges such inputs away and every case asserts that none is left; no element is ever excluded from a comparison.

Convention at n = 1: the unbiased factor of running_var is n / max(n - 1, 1), i.e. 1 - the kernels' convention where nn.BatchNorm
raises ("Expected more than 1 value per channel").
"""
import math
import os
from collections import namedtuple

import torch

if os.environ.get("S2D_ROW_RPT") is not None:
    raise RuntimeError("S2D_ROW_RPT is set in the environment: the library would take another row plan than the one mirrored in "
                       "tests/bn_pass_ref.py (8 rows per thread).  Unset it to run the batch-norm pass tests.")

ROW_RPT = 8
RED_THREADS = 256
ROW_UNROLL = 4
ROW_REDUCE_CAP, ROW_LAUNCH_CAP, RED_CAP, BN_APPLY_CAP, CM_APPLY_CAP = 2048, 16384, 1024, 4096, 1024
PS_LONG, PS_SLICES = 1536, 512
S2D_OK, S2D_ERR_INVALID_ARG, S2D_ERR_UNSUPPORTED, S2D_ERR_WORKSPACE = 0, -1, -2, -4

E_ACT_MEASURED = 4.5e-7   # measured 4.474e-7 on the MI355X, rounded up
E_ACT_FACTOR = 4.0
E_ACT = E_ACT_FACTOR * E_ACT_MEASURED

GUARD = 2   # guard rows on each side of a caller-owned buffer
U32 = 2.0 ** -24


def ceil_div(a, b):
    return -(-a // b)


def align_up(v, a):
    return ceil_div(v, a) * a


# ---- plan mirrors -------------------------------------------------------------------------------------------------------------------
RedPlan = namedtuple("RedPlan", "nblocks rows_per_block lanes empty ws_bytes")
RowLaunch = namedtuple("RowLaunch", "blocks threads lanes trips")
CmPlan = namedtuple("CmPlan", "chunks chunk4 ws_bytes")
PartialsPlan = namedtuple("PartialsPlan", "prefold rows_per_slice slices ws_bytes")


def _red(n, lanes, rows_per_thread, cap, c):
    rows = max(n, 1)
    nb = min(ceil_div(rows, lanes * rows_per_thread), cap)
    rpb = ceil_div(rows, nb)
    return RedPlan(nb, rpb, lanes, nb - ceil_div(rows, rpb), align_up(nb * 2 * c * 4, 256))


def row_plan_bf16(n, c):
    """row_plan_bf16 of features.hip: the reduce launches of the row-major bf16 entries; .empty = trailing workgroups with r0 >= n"""
    return _red(n, max(RED_THREADS // (c // 8), 1), ROW_RPT, ROW_REDUCE_CAP, c)


def red_plan(n, c):
    """red_plan of features.hip: the reduce launches of the row-major fp32 entries (16 rows per lane, at most 1024 workgroups)"""
    return _red(n, max(RED_THREADS // (c // 4), 1), 16, RED_CAP, c)


def row_launch(n, c):
    """row_launch of features.hip: the apply / backward-apply launches of the row-major bf16 entries; .trips of 4 rows per thread"""
    c8 = c // 8
    lanes = max(256 // c8, 1)
    blocks = min(ceil_div(n, lanes * ROW_UNROLL), ROW_LAUNCH_CAP)
    return RowLaunch(blocks, lanes * c8, lanes, ceil_div(n, blocks * lanes * ROW_UNROLL))


def bn_apply_trips(n, c):
    """grid-stride trips of bn_apply_kernel / bn_bwd_apply_kernel (one float4 per thread and trip, at most 4096 workgroups)"""
    n4 = n * (c // 4)
    return ceil_div(n4, min(ceil_div(n4, 256), BN_APPLY_CAP) * 256)


def cm_plan(batch, c, positions):
    p4 = positions // 4
    chunks = max(min(ceil_div(2048, c), ceil_div(p4, 1024)), 1)
    return CmPlan(chunks, ceil_div(p4, chunks), align_up(chunks * 2 * c * 4, 256))


def cm_apply_trips(positions):
    p4 = positions // 4
    return ceil_div(p4, min(ceil_div(p4, 256), CM_APPLY_CAP) * 256)


def partials_plan(nblocks, c, with_ws=True):
    """the prefold of a partial list: engaged exactly when nblocks > PS_LONG, 2c <= 256 and the caller passes the workspace"""
    if nblocks <= PS_LONG or 2 * c > 256:
        return PartialsPlan(False, 0, nblocks, 0)
    ws = align_up(PS_SLICES * 2 * c * 4, 256)
    if not with_ws:
        return PartialsPlan(False, 0, nblocks, ws)
    rps = ceil_div(nblocks, PS_SLICES)
    return PartialsPlan(True, rps, ceil_div(nblocks, rps), ws)


# chain lengths L of the sums bound
def fold_sum(nblocks):        # partial_sum_kernel: one wave per element, 6 butterfly steps
    return ceil_div(nblocks, 64) + 6


def fold_finalize(nblocks):   # bn_reduce_finalize_*_kernel: 256 threads per channel, 6 butterfly steps + 2 LDS steps
    return ceil_div(nblocks, 256) + 8


def chain_rows(plan, fold):
    return ceil_div(plan.rows_per_block, plan.lanes) + plan.lanes + fold(plan.nblocks)


def chain_cm(batch, plan, fold=fold_sum):
    """cm_reduce_kernel: per thread batch * ceil(chunk4 / 256) trips of (2-step tree, 1 accumulate), 6 butterfly + 2 LDS steps"""
    return batch * ceil_div(plan.chunk4, 256) + 2 + 8 + fold(plan.chunks)


def chain_partials(nblocks, c, with_ws, fold):
    p = partials_plan(nblocks, c, with_ws)
    if not p.prefold:
        return fold(nblocks)
    lanes = 256 // (2 * c)
    return ceil_div(p.rows_per_slice, lanes) + 2 + lanes + fold(p.slices)


# ---- ulps -----------------------------------------------------------------------------------------------------------------------------
def _ulp(v, mant_bits, min_exp):
    v = torch.as_tensor(v, dtype=torch.float64).abs()
    _, e = torch.frexp(v)                                        # v = f * 2^e, f in [0.5, 1)
    e = torch.where(v > 0, e, torch.full_like(e, min_exp)).clamp_min(min_exp + mant_bits + 1)
    return torch.ldexp(torch.ones_like(v), e - (mant_bits + 1))


def ulp_fp32(v):
    return _ulp(v, 23, -149)


def ulp_bf16(v):
    return _ulp(v, 7, -133)


# ---- float64 restatements (on the stored operands) -------------------------------------------------------------------------------------
_RSQRT2 = 0.70710678118654752
_RSQRT2PI = 0.3989422804014327


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z * _RSQRT2))


def gelu_grad64(z):
    return 0.5 * (1.0 + torch.erf(z * _RSQRT2)) + z * _RSQRT2PI * torch.exp(-0.5 * z * z)


def gelu_f32(v):
    """gelu_f of s2d_common.h with torch's fp32 erf (the yardstick of E_ACT and the host emulation)"""
    return 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))


def gelu_grad_f32(v):
    return 0.5 * (1.0 + torch.erf(v * 0.70710678118654752)) + v * 0.3989422804014327 * torch.exp(-0.5 * v * v)


def gelu_yardstick(device, points=2_000_001):
    """largest |fp32 closed form with torch's erf / exp - float64| over z in [-10, 10], for gelu_f and gelu_grad_f"""
    z = torch.linspace(-10, 10, points, dtype=torch.float64, device=device).float()
    z64 = z.double()
    return max(float((gelu_f32(z).double() - gelu64(z64)).abs().max()), float((gelu_grad_f32(z).double() - gelu_grad64(z64)).abs().max()))


def ref_sums(x, dim=0):
    """-> (sums [2c] = (sum x, sum x^2), the sums of the terms' magnitudes [2c]) over the rows of x [n, c]"""
    x = x.double()
    s1 = (x * x).sum(dim)
    return torch.cat([x.sum(dim), s1]), torch.cat([x.abs().sum(dim), s1])


def ref_z(x, scale, shift):
    """-> (z = x scale + shift, |x scale| + |shift|) in float64; scale / shift broadcast over the rows"""
    xs = x.double() * scale.double()
    return xs + shift.double(), xs.abs() + shift.double().abs()


def ambiguous(x, scale, shift):
    z, mag = ref_z(x, scale, shift)
    return (z != 0) & (z.abs() < 2.0 ** -20 * mag)


def make_unambiguous(x, scale, shift):
    """nudges the elements of x (in place, in its own dtype) whose mask fma(x, scale, shift) > 0 is ambiguous; -> the count left (0)"""
    for _ in range(4):
        amb = ambiguous(x, scale, shift)
        if not bool(amb.any()):
            return 0
        x[amb] = (x[amb].float() * 1.5 + 0.25).to(x.dtype)
    return int(ambiguous(x, scale, shift).sum())


def ref_g(dy, act, z=None, y=None):
    """g = dy * act'(.) in float64 and the activation term of its bound.  act 0: dy; 1: the mask y > 0 (y given) or z > 0; 2: GELU'(z)"""
    dy = dy.double()
    if act == 0:
        return dy, torch.zeros_like(dy)
    if act == 1:
        on = (y.double() > 0) if y is not None else (z > 0)
        return torch.where(on, dy, torch.zeros_like(dy)), torch.zeros_like(dy)
    return dy * gelu_grad64(z), E_ACT * z.abs().clamp_min(1.0) * dy.abs()


def ref_bwd_sums(g, g_err, x, dim=0):
    """-> (sums [2c] = (sum g, sum g x), sums of the magnitudes, the summed activation terms)"""
    x = x.double()
    gx = g * x
    return (torch.cat([g.sum(dim), gx.sum(dim)]), torch.cat([g.abs().sum(dim), gx.abs().sum(dim)]),
            torch.cat([g_err.sum(dim), (g_err * x.abs()).sum(dim)]))


def ref_apply(x, scale, shift, res, act):
    """y = act(x scale + shift [+ res]) -> (ref, M, activation term)"""
    z, mag = ref_z(x, scale, shift)
    if res is not None:
        z, mag = z + res.double(), mag + res.double().abs()
    if act == 1:
        return z.clamp_min(0.0), mag, torch.zeros_like(z)
    if act == 2:
        return gelu64(z), mag, E_ACT * z.abs().clamp_min(1.0)
    return z, mag, torch.zeros_like(z)


def ref_bwd_apply(g, g_err, x, a, b, d):
    """dx = a g + b x + d -> (ref, M, activation term)"""
    ag, bx = a.double() * g, b.double() * x.double()
    return ag + bx + d.double(), ag.abs() + bx.abs() + d.double().abs(), a.double().abs() * g_err


def _big(*ts):
    shape = torch.broadcast_shapes(*[t.shape for t in ts])
    return torch.stack([t.abs().expand(shape) for t in ts]).amax(0)


def fwd_finalize(s0, s1, n, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """the forward finalize in float64 -> {name: (value, m)}, m = the largest intermediate of that output's formula.
    unbiased factor n / max(n - 1, 1): the kernels' convention at n = 1, where nn.BatchNorm raises"""
    s0, s1, gamma, beta = s0.double(), s1.double(), gamma.double(), beta.double()
    mean, ex2 = s0 / n, s1 / n
    var = (ex2 - mean * mean).clamp_min(0.0)
    invstd = torch.rsqrt(var + eps)
    scale = gamma * invstd
    ms = mean * scale
    m_is = _big(ex2, mean * mean, var + eps, invstd)
    out = {"mean": (mean, mean.abs()), "invstd": (invstd, m_is), "scale": (scale, _big(m_is, scale)),
           "shift": (beta - ms, _big(m_is, scale, beta, ms))}
    if running_mean is not None:
        rm, rv = running_mean.double(), running_var.double()
        unbiased = var * (n / max(n - 1.0, 1.0))
        out["running_mean"] = ((1.0 - momentum) * rm + momentum * mean, _big(rm, mean))
        out["running_var"] = ((1.0 - momentum) * rv + momentum * unbiased, _big(rv, ex2, mean * mean, unbiased))
    return out


def bwd_finalize_local(sg, sgx, mean, invstd):
    """dgamma, dbeta of the backward finalize: functions of the LOCAL sums alone"""
    sg, sgx, mean, invstd = sg.double(), sgx.double(), mean.double(), invstd.double()
    dg = invstd * (sgx - mean * sg)
    return {"dbeta": (sg, sg.abs()), "dgamma": (dg, _big(sgx, mean * sg, dg))}


def bwd_finalize_global(sg, sgx, n, gamma, mean, invstd):
    """a, b, d of the backward finalize: functions of the GLOBAL sums and the global count (what a SyncBN all-reduce hands over)"""
    sg, sgx, gamma, mean, invstd = sg.double(), sgx.double(), gamma.double(), mean.double(), invstd.double()
    dg = invstd * (sgx - mean * sg)
    a = gamma * invstd
    b = -(a * invstd) * dg / n
    t0, t1 = -(a * sg) / n, b * mean
    m_b = _big(sgx, mean * sg, dg, a * invstd, a * invstd * dg, b)
    return {"a": (a, a.abs()), "b": (b, m_b), "d": (t0 - t1, _big(m_b, a * sg, t0, t1))}


# ---- checkers -------------------------------------------------------------------------------------------------------------------------
WORST = {}   # family -> the worst observed error as a fraction of its bound (what profiles/bn_pass_parity.txt reports)


def _note(family, err, bound):
    if family is None or err.numel() == 0:
        return
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, math.inf, 0.0).to(err.dtype))
    WORST[family] = max(WORST.get(family, 0.0), float(torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf).max()))


def _fail(what, bad, names):
    idx = bad.nonzero()
    raise AssertionError(f"{what}: {int(idx.shape[0])} of {bad.numel()} elements outside the bound; first ({names}): {idx[:8].tolist()}")


def check_elementwise(out, ref, mag, act_term=None, what="out", family=None, names="row, channel"):
    """|out - ref| <= [1/2 ulp_bf16(ref) if out is bf16] + 4 ulp_fp32(M) [+ the activation term]; a NaN is a miss"""
    bound = 4.0 * ulp_fp32(mag)
    if out.dtype == torch.bfloat16:
        bound = bound + 0.5 * ulp_bf16(ref)
    if act_term is not None:
        bound = bound + act_term
    err = (out.double() - ref).abs()
    _note(family, err, bound)
    if out.dtype == torch.bfloat16 and family is not None:
        # a bf16 tie reads 1.000 above by nature; what is left of the error after the one rounding, as a share of the other terms
        half = 0.5 * ulp_bf16(ref)
        _note(family + ", beyond the bf16 rounding", (err - half).clamp_min(0.0), bound - half)
    bad = ~(err <= bound)
    if bool(bad.any()):
        _fail(what, bad, names)


def _raw(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def check_bits(out, ref, what="out", names="row, channel"):
    """out is bit-equal to ref (same dtype)"""
    assert out.dtype == ref.dtype and out.shape == ref.shape, (what, out.dtype, ref.dtype, tuple(out.shape), tuple(ref.shape))
    bad = _raw(out) != _raw(ref)
    if bool(bad.any()):
        _fail(what + " (bit comparison)", bad, names)


def check_sums(s, ref, mag, chain, act_term=None, what="sums", family=None):
    """|s - ref| <= chain * 2^-24 * sum|term| [+ the summed activation terms] per element of the [2c] vector; -> the bound"""
    bound = chain * U32 * mag
    if act_term is not None:
        bound = bound + act_term
    err = (s.double() - ref).abs()
    _note(family, err, bound)
    bad = ~(err <= bound)
    if bool(bad.any()):
        c = ref.numel() // 2
        idx = bad.nonzero().flatten()[:8].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} sums outside {chain} * 2^-24 * sum|term|; first (vector, channel): "
                             f"{[(i // c, i % c) for i in idx]}, |err| / bound {[float(err[i] / bound[i]) if bound[i] > 0 else math.inf for i in idx]}")
    return bound


def check_box(dev, fn, s0, d0, s1, d1, what="finalize", family=None, apart=None):
    """every per-channel output dev[name] lies inside the range the float64 formula fn(s0, s1) -> {name: (value, m)} takes at the
    four corners of [s0 +- d0] x [s1 +- d1], widened by 8 ulp_fp32(m).  apart (bool per channel): channels whose share of the box is
    noted under their own name - a clamped variance sits on the box's corner by construction and says nothing about the others"""
    centre = fn(s0, s1)
    corners = [fn(s0 + i * d0, s1 + j * d1) for i in (-1, 1) for j in (-1, 1)]
    assert set(dev) == set(centre), (what, sorted(dev), sorted(centre))
    for name, got in dev.items():
        vals = torch.stack([cn[name][0] for cn in corners] + [centre[name][0]])
        slack = 8.0 * ulp_fp32(centre[name][1])
        lo, hi = vals.amin(0) - slack, vals.amax(0) + slack
        g = got.double()
        off, half = (g - 0.5 * (hi + lo)).abs(), 0.5 * (hi - lo)
        if apart is None or family is None:
            _note(family, off, half)
        else:
            _note(family, off[~apart], half[~apart])
            _note(family + ", channels without variance or with gamma = 0", off[apart], half[apart])
        bad = ~((g >= lo) & (g <= hi))
        if bool(bad.any()):
            idx = bad.nonzero().flatten()[:8].tolist()
            raise AssertionError(f"{what}: {name} outside its box at {int(bad.sum())} of {bad.numel()} channels; first channels {idx}, "
                                 f"device {[float(g[i]) for i in idx]}, box {[(float(lo[i]), float(hi[i])) for i in idx]}")


def old_criterion(out, ref):
    """the per-tensor criterion of the module-level tests (1e-2 * max|ref|), kept to show what it lets through"""
    return bool(((out.double() - ref).abs() <= 1e-2 * ref.abs().max()).all())


# ---- buffers ----------------------------------------------------------------------------------------------------------------------------
def poisoned(rows, *row_shape, dtype, device):
    """-> (the whole allocation, its rows [GUARD : GUARD + rows] that the launch may write), all of it NaN"""
    buf = torch.full((rows + 2 * GUARD,) + tuple(row_shape), float("nan"), dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + rows]


def _fill_bits(dtype, device):
    return _raw(torch.full((1,), float("nan"), dtype=dtype, device=device)).item()


def assert_guards(buf, what):
    """the guard rows of a `poisoned` allocation still hold the fill bit for bit"""
    fill = _fill_bits(buf.dtype, buf.device)
    bits = _raw(buf).reshape(buf.shape[0], -1)
    for name, g in (("front", bits[:GUARD]), ("back", bits[-GUARD:])):
        assert bool((g == fill).all()), f"{what}: {name} guard rows overwritten ({int((g != fill).sum())} elements)"


def assert_written(buf, what):
    """guards bit-unchanged, everything between them finite"""
    assert_guards(buf, what)
    body = buf[GUARD:-GUARD].reshape(buf.shape[0] - 2 * GUARD, -1)
    unwritten = (~torch.isfinite(body)).any(1)
    assert not bool(unwritten.any()), (f"{what}: rows left at the NaN fill", int(unwritten.sum()), unwritten.nonzero().flatten()[:8].tolist())


def assert_untouched(buf, what):
    """the whole allocation still holds the fill: the entry returned before any launch"""
    bits = _raw(buf)
    assert bool((bits == _fill_bits(buf.dtype, buf.device)).all()), f"{what}: written although the entry refused the call"


def wide(rows, c, ld, dtype, device):
    """a channel slice [rows, c] of a wider row-major tensor [rows + guards, ld], all of it NaN -> (allocation, slice, column offset).
    The offset keeps the slice 16-byte aligned; with ld == c it is the plain contiguous buffer"""
    off = 0 if ld == c else (8 if ld - c < c else c)
    buf = torch.full((rows + 2 * GUARD, ld), float("nan"), dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + rows, off:off + c], off


def assert_slice_written(buf, off, c, what):
    """only the slice's columns of the body rows were written: they are finite, every other element keeps the fill bit for bit"""
    fill = _fill_bits(buf.dtype, buf.device)
    bits = _raw(buf)
    outside = torch.ones_like(bits, dtype=torch.bool)
    outside[GUARD:-GUARD, off:off + c] = False
    touched = outside & (bits != fill)
    if bool(touched.any()):
        _fail(what + ": elements outside the destination slice overwritten", touched, "allocation row, column")
    body = buf[GUARD:-GUARD, off:off + c]
    unwritten = (~torch.isfinite(body)).any(1)
    assert not bool(unwritten.any()), (f"{what}: rows left at the NaN fill", int(unwritten.sum()), unwritten.nonzero().flatten()[:8].tolist())


# ---- case tables (the edge shapes come from the mirrors) ------------------------------------------------------------------------------
def row_tails(lanes, rows_per_thread=ROW_RPT):
    """row counts that each hit another tail of the 4-row / 8-row unrolled trips, and one with two full workgroups and a ragged third"""
    full = lanes * rows_per_thread
    ns = [1, lanes - 1, lanes + 1, 4 * lanes + 1, 8 * lanes * 3 - 5, 2 * full + 3 * lanes + 1]
    return sorted({n for n in ns if n > 0})


ROW_C = (8, 24, 64, 128, 136, 200, 1016, 1024)
ROW = {
    "entries": ("s2d_bnrow_workspace_bytes", "s2d_bnrow_stats_bf16", "s2d_bnrow_stats_finalize_bf16", "s2d_bnrow_apply_bf16",
                "s2d_bnrow_apply_ld_bf16", "s2d_bnrow_bwd_reduce_bf16", "s2d_bnrow_bwd_reduce_ld_bf16",
                "s2d_bnrow_bwd_reduce_finalize_bf16", "s2d_bnrow_bwd_reduce_finalize_ld_bf16", "s2d_bnrow_bwd_apply_bf16",
                "s2d_bnrow_bwd_apply_ld_bf16"),
    "cases": [(c, n) for c in ROW_C for n in row_tails(row_plan_bf16(1, c).lanes)],
    "reduce_cap": [(1024, 32769), (512, 3 * 2048 * 4 * 8 + 5)],
    "apply_cap": (1024, 131073),
    "fused_vs_split": [(24, row_tails(row_plan_bf16(1, 24).lanes)[3]), (136, row_tails(row_plan_bf16(1, 136).lanes)[-1]),
                       (1024, row_tails(row_plan_bf16(1, 1024).lanes)[-2])],
    # (what, c, n, y_ld - c, workspace bytes short, relu) -> the documented code
    "refused": [("c = 12", 12, 40, 0, 0, 1, S2D_ERR_UNSUPPORTED), ("c = 1032", 1032, 40, 0, 0, 1, S2D_ERR_UNSUPPORTED),
                ("n = 0", 64, 0, 0, 0, 1, S2D_ERR_INVALID_ARG), ("y_ld = c + 4", 64, 40, 4, 0, 1, S2D_ERR_INVALID_ARG),
                ("workspace one byte short", 64, 40, 0, 1, 1, S2D_ERR_WORKSPACE), ("relu = 3", 64, 40, 0, 0, 3, S2D_ERR_INVALID_ARG)],
}


def row_lds(c):
    return (c, c + 8, 3 * c)


BN1D_C = (4, 16, 100, 128, 1024)
BN1D = {
    "entries": ("s2d_bn1d_workspace_bytes", "s2d_bn1d_stats_f32", "s2d_bn1d_finalize_fwd_f32", "s2d_bn1d_finalize_bwd_f32",
                "s2d_bn1d_stats_finalize_f32", "s2d_bn1d_bwd_reduce_finalize_f32", "s2d_bn1d_apply_f32", "s2d_bn1d_bwd_reduce_f32",
                "s2d_bn1d_bwd_apply_f32"),
    "cases": [(c, n) for c in BN1D_C for n in row_tails(red_plan(1, c).lanes, 16)],
    "reduce_cap": (1024, 16385),
    "apply_cap": (1024, 4097),
}

CM = {
    "entries": ("s2d_bncm_workspace_bytes", "s2d_bncm_stats_f32", "s2d_bncm_apply_f32", "s2d_bncm_bwd_reduce_f32",
                "s2d_bncm_bwd_reduce_x_f32", "s2d_bncm_bwd_apply_f32", "s2d_bncm_bwd_apply_x_f32", "s2d_bncm_bwd_reduce_x_typed",
                "s2d_bncm_bwd_apply_x_typed"),
    "cases": [(b, c, p) for b, c in ((1, 1), (3, 3), (2, 16), (4, 32)) for p in (4, 1020, 4100)],
    "chunks_by_channels": (1, 32, 4 * (ceil_div(2048, 32) * 1024 + 1024 + 3)),   # ceil(2048 / c) = 64 < ceil(p4 / 1024) = 66
    "apply_cap": (1, 1, 4 * 262145),
    "typed": [(0, 0, 0), (1, 0, 0), (1, 1, 1)],   # the supported (dy_bf16, x_bf16, dx_bf16)
    "rejected_positions": 6,
}

PARTIALS = {
    "entries": ("s2d_bn_partials_sum_workspace_bytes", "s2d_bn_partials_finalize_ws_f32", "s2d_bn_partials_finalize_f32",
                "s2d_bn_partials_bwd_finalize_ws_f32", "s2d_bn_partials_sum_ws_f32", "s2d_bn_partials_sum_f32"),
    "cases": [(nb, c) for nb in (1, 255, 257, PS_LONG, PS_LONG + 1, 4500, 70000) for c in (16, 24, 128, 136)],
}

TABLES = {"row-major bf16": ROW, "row-major fp32": BN1D, "channel-major": CM, "partial lists": PARTIALS}
PREFIXES = ("s2d_bn1d_", "s2d_bnrow_", "s2d_bncm_", "s2d_bn_partials_")
CALLED = set()


def table_entries():
    return {name for t in TABLES.values() for name in t["entries"]}


def entry(lib, name):
    """the library's entry `name`; only names of the case tables may be called, and what was called is recorded"""
    assert name in table_entries(), f"{name} is not in a case table of tests/bn_pass_ref.py"
    CALLED.add(name)
    return getattr(lib, name)


# ---- host emulations (torch fp32 arithmetic, bf16 round-to-nearest stores): what the CPU checks feed the checkers ---------------------
def emu_apply(x, scale, shift, res, act, out_dtype):
    v = x.float() * scale + shift
    if res is not None:
        v = v + res.float()
    if act == 1:
        v = v.clamp_min(0.0)
    if act == 2:
        v = gelu_f32(v)
    return v.to(out_dtype)


def emu_g(dy, x, scale, shift, act, y=None):
    g = dy.float()
    if act == 1:
        on = (y.float() > 0) if y is not None else (x.float() * scale + shift > 0)
        g = torch.where(on, g, torch.zeros_like(g))
    if act == 2:
        g = g * gelu_grad_f32(x.float() * scale + shift)
    return g


def emu_bwd_apply(g, x, a, b, d, out_dtype):
    return (a * g + (b * x.float() + d)).to(out_dtype)


def emu_block_partials(t, plan):
    """[nblocks, width] fp32 partial rows of t [n, width] under a reduce plan (empty trailing workgroups write zeros)"""
    rows = [t[b * plan.rows_per_block:(b + 1) * plan.rows_per_block].float().sum(0) for b in range(plan.nblocks)]
    return torch.stack(rows)


def emu_fwd_finalize(s0, s1, n, gamma, beta, eps, momentum, rm=None, rv=None):
    n = torch.tensor(float(n), dtype=torch.float32)
    mean = s0 / n
    var = (s1 / n - mean * mean).clamp_min(0.0)
    invstd = torch.rsqrt(var + eps)
    sc = gamma * invstd
    out = {"mean": mean, "invstd": invstd, "scale": sc, "shift": beta - mean * sc}
    if rm is not None:
        unbiased = var * (n / torch.clamp(n - 1.0, min=1.0))
        out["running_mean"] = (1.0 - momentum) * rm + momentum * mean
        out["running_var"] = (1.0 - momentum) * rv + momentum * unbiased
    return out


def emu_bwd_finalize(sl0, sl1, sg0, sg1, n, gamma, mean, invstd):
    n = torch.tensor(float(n), dtype=torch.float32)
    dg_all = invstd * (sg1 - mean * sg0)
    av = gamma * invstd
    bv = -(av * invstd) * dg_all / n
    return {"dbeta": sl0.clone(), "dgamma": invstd * (sl1 - mean * sl0), "a": av, "b": bv, "d": -(av * sg0) / n - bv * mean}
