"""TEST INFRASTRUCTURE ONLY - float64 restatements, error bounds, checkers, case tables and an fp32 host emulation for the fused
PointPillars feature net of csrc/pfn.hip (the 13 s2d_pfn_* / s2d_pfn2_* entries).  Imports without a GPU and never loads the native
library: tests/test_pfn_parity_gpu.py drives the entries, tests/test_pfn_checks_cpu.py shows on the host that every checker can fail.

Formulas (the header comments of csrc/pfn.hip, PillarFeatureNet.forward / PFNLayer.forward), on the fp32 inputs as given:
  n = clamp(num, 0, T); slot t < n is valid, every other slot is EMPTY and carries f = 0 (a pillar with n = 0 is all empty slots, its
  mean is not used);  mean = (sum of x, y, z over all T slots) / n;  centre = coors[:, 3] * vx + x_offset, coors[:, 2] * vy + y_offset;
  f = (x, y, z, i, e, x - mean_x, y - mean_y, z - mean_z, x - centre_x, y - centre_y);  h = W f;  y = relu(h * scale + shift);
  out = max over the T slots, arg = the first maximum (an empty slot counts as slot n).
  Two layers: h1 = W1 f (32), x1 = relu(bn1(h1)), m1 = max x1, h2 = W2 [x1 | m1], y2 = relu(bn2(h2)), out = max y2.

Bounds.  Nothing below is fitted to what the kernels return.  u = 2^-24, gamma(k) = k u / (1 - k u).  Every bound has the form
      |x - ref| <= (errors propagated from the operands) + gamma(chain) * sum |term|
  with the magnitude companion sum |term| = the same reference evaluated on absolute values, and chain = the number of fp32 roundings on
  the longest path into one accumulator, counted from the kernel:
    decorations   x - mean: at most n - 1 additions and one division for the mean, one subtraction -> chain T + 1 on |p| + sum|p| / n
                  x - centre: one product, one addition, one subtraction -> chain 3 on |p| + |c v| + |offset|     (not on |f|)
    h, h1         10 fma from zero -> e(h) = |W| e(f) + gamma(10) |W| |f|mag
    y, x1         one fma -> e = |scale| e(h) + gamma(1) (|scale| |h|mag + |shift|); an empty slot's relu(shift) is exact
    m1, out       |max a - max b| <= max |a_t - b_t| over the slots that take part
    h2            32 + 32 fma -> e(h2) = |A| e(x1) + |B| e(m1) + gamma(64) (|A| x1 + |B| m1)
    sums          pfn_stats / pfn2_stats2: one wave adds trips * T rows, the block fold adds 2 levels -> chain trips * T + 2 (the square of
                  pfn2_stats2 rounds mult * h2 first: + 1); pfn2_stats1: a half-wave adds trips * ceil(T / 2) rows, one half-wave fold,
                  2 levels -> trips * ceil(T / 2) + 3.  trips = ceil(P / (4 blocks)).
    pfn_bwd       sum g, sum g h, M1: one non-zero term per pillar and channel -> trips + 2; M2, M3: trips * T + 2
    pfn2_bwd      dh2 = fma(a, g, [T - n] * fma(b, h2, d)): chain 3; sum of dh2 over the rows: T; dW2[:, :32]: trips2 * T fma; dW2[:, 32:]:
                  trips2 fma; dm1, dz: 64 fma; gin = dz + dm1: 1; layer-1 sums: a half-wave adds trips2 * ceil(T / 2) rows + one fold.
                  trips2 = ceil(P / 1024).
  Products of two inexact factors carry e(a) |b|mag + |a|mag e(b) + e(a) e(b).

Argmax.  arg passes when y_ref[arg] >= max y_ref - (e[arg] + e_max) (the kernel compared two computed values, each off by its own bound;
e_max = the largest bound over the slots that take part) and out is within e_max of max y_ref.  Where the float64 gap between the top
two values is exactly 0 or above 2 e_max, arg must equal the float64 first maximum; at least 95 % of the (pillar, channel) pairs of every
case must fall under that strict rule (asserted).

pfn2_bwd recomputes the layer-1 argmax and the layer-1 ReLU gate.  Ref2.rejected() names, in float64, every pillar with a valid
|h1 sc1 + sh1| < tau or a top-two gap of x1 strictly inside (0, tau), tau = 1e-4 max |h1 sc1 + sh1|; screened_case() redraws those
pillars until none is left (at most 12 rounds, else it raises) and asserts tau > 2 max e(x1), so that both decisions are the float64
ones by derivation.  Exact ties (duplicated points) stay: the first slot wins in either precision.

The references also accept how far the kernel's copy of scale / shift, abd2 or the output gradient may lie from the float64 one
(prm.e_scale, e_shift, e_ss1, e_ss2; e_abd2, e_gout, e_g) and then carry both outcomes of a decision that lies within its own bound:
that is what ModuleRef (PillarFeatureNet on top of the entries) feeds them, its batch-norm vectors coming out of an fp32 finalisation.
The entry-level suites own those inputs and leave all of them at zero.

ModuleRef and the two-layer reader in TRAIN mode.  Every gradient and output is asserted against its propagated bound there too, but the
bounds of the first layer's gradients are vacuous (tens to hundreds of times the value), and this cannot be derived away in a worst-case
analysis: e(mean2) is the AVERAGE of e(h2) over all rows, about 1e-3 (|B| e(m1) with e(m1) = e(scale1) |h1|), because worst-case
errors add coherently; against std(h2) of about 0.5 that is 0.2 .. 0.8 % on scale2 and shift2 and, after the backward finalisation, on
b2 and d2.  The terms b2 h2 + d2 of dh2 reach every one of the P T rows and cancel in exact arithmetic (batch norm's backward sums to
zero) but not in magnitude, so dz, the layer-1 sums and dW1 inherit P T |e(b2) h2 + e(d2)| against a true value that is a difference.
What is tight there: the running statistics of both layers and num_batches_tracked; out is held to about 1e-2 absolute.  The one-layer
reader in both modes and the two-layer reader in eval mode have meaningful bounds throughout; profiles/pfn_parity.txt lists the median
of bound / |reference| per family (the largest over the cases, which is the P = 1 case with its statistics over 13 or 20 rows).
"""
import math
import types

import torch

from bn_pass_ref import GUARD, U32, WORST, _note, assert_guards, assert_written, ceil_div, check_bits, poisoned  # noqa: F401

C, C1, F, T_MAX = 64, 32, 10, 20
BWD_COLS = (2 + 2 * F) * C + F
BWD2_COLS = C * C + BWD_COLS
BWD2_ROWS = 1024
STRICT_SHARE = 0.95
TAU_REL = 1e-4
REDRAW_ROUNDS = 12


def f32(v):
    """the fp32 value the entry receives for a float argument"""
    return float(torch.tensor(v, dtype=torch.float32))


# the Waymo pillar geometry (configs/waymo/pp/*): voxel 0.32, range -74.88 .. 74.88, a 468 x 468 grid
GEO = (f32(0.32), f32(0.32), f32(0.32 / 2 - 74.88), f32(0.32 / 2 - 74.88))
GRID = 468
POINT_SCALES = (20.0, 20.0, 1.5, 0.5, 0.1)


def gamma(k):
    return k * U32 / (1.0 - k * U32)


def blocks_mirror(pillars):
    """pfn_blocks of pfn.hip (the GPU tests size their buffers from s2d_pfn_blocks and assert that it equals this)"""
    return min(max(ceil_div(pillars, 4), 1), 1024)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
T_AXIS = (1, 2, 12, 13, 19, 20)
P_AXIS = (1, 3, 4, 5, 1023, 1025, 4096, 4097, 9001)
CASES = sorted({(p, t) for p in P_AXIS for t in (13, 20)} | {(p, t) for t in T_AXIS for p in (5, 4097)})
FORCED_NUM = ("T", 0, 1, "T+3", -1)
ADVERSARIAL_ARG = ("valid", "n", "above_n", "last", "zero")
ABD2 = ("train", "eval")
ENTRIES = {
    "one layer": ("s2d_pfn_supported", "s2d_pfn_blocks", "s2d_pfn_bwd_cols", "s2d_pfn_stats_f32", "s2d_pfn_apply_max_f32", "s2d_pfn_bwd_f32"),
    "two layers": ("s2d_pfn2_supported", "s2d_pfn2_bwd_rows", "s2d_pfn2_bwd_cols", "s2d_pfn2_stats1_f32", "s2d_pfn2_stats2_f32",
                   "s2d_pfn2_apply_max_f32", "s2d_pfn2_bwd_f32"),
}
CALLED = set()


def table_entries():
    return {n for names in ENTRIES.values() for n in names}


def entry(lib, name):
    assert name in table_entries(), f"{name} is not in the entry table of tests/pfn_ref.py"
    CALLED.add(name)
    return getattr(lib, name)


def seed_of(pillars, slots):
    return 1000 * slots + pillars % 997


def _draw_points(case, which, g):
    """fresh points for the pillars `which` (host tensors): duplicated-point pillars repeat one point, empty slots stay zero"""
    t = case.T
    pts = torch.randn(which.numel(), t, 5, generator=g) * torch.tensor(POINT_SCALES)
    dup = case.dup[which]
    pts[dup] = pts[dup][:, :1].expand(-1, t, -1).clone()
    n = case.num[which].clamp(0, t)
    case.vox[which] = pts * (torch.arange(t)[None, :] < n[:, None])[:, :, None]


def make_case(pillars, slots, seed=None):
    """host tensors.  num_points: a uniform draw over 0..T, then about half of the pillars (all of them below 10) forced cyclically to
    T, 0, 1, T + 3 and -1; every fourth pillar of a random order holds one point duplicated over its n slots (exact ties)"""
    g = torch.Generator().manual_seed(seed_of(pillars, slots) if seed is None else seed)
    t = slots
    num = torch.randint(0, t + 1, (pillars,), generator=g, dtype=torch.int32)
    order = torch.randperm(pillars, generator=g)
    forced = [t, 0, 1, t + 3, -1]
    take = min(pillars, 5 * max(1, pillars // 10))
    for j in range(5):
        num[order[j:take:5]] = forced[j]
    dup = torch.zeros(pillars, dtype=torch.bool)
    dup[order[3::4]] = True
    coors = torch.stack([torch.randint(0, 4, (pillars,), generator=g), torch.zeros(pillars, dtype=torch.int64),
                         torch.randint(0, GRID, (pillars,), generator=g), torch.randint(0, GRID, (pillars,), generator=g)], 1).int()
    case = types.SimpleNamespace(P=pillars, T=t, num=num, dup=dup, coors=coors, vox=torch.zeros(pillars, t, 5), geo=GEO, gen=g, rounds=0,
                                 first_reject=0.0)
    _draw_points(case, torch.arange(pillars), g)
    return case


def case_to(case, device):
    out = types.SimpleNamespace(**vars(case))
    out.vox, out.num, out.coors, out.dup = case.vox.to(device), case.num.to(device), case.coors.to(device), case.dup.to(device)
    return out


ZERO_CHANNELS = (7, 39)       # scale 1e-3, shift -1: every output of the channel is 0 (|h| stays far below 1000)
NEG_SCALE_EVERY = 4           # channels c % 4 == 1 have a negative scale; even channels a positive shift, odd ones a negative shift


def _scale_shift(c, g):
    scale = (torch.rand(c, generator=g) + 0.5) * 0.1
    scale[1::NEG_SCALE_EVERY] *= -1.0
    shift = (torch.randn(c, generator=g) * 0.5).abs() + 0.01
    shift[1::2] *= -1.0
    for z in ZERO_CHANNELS:
        if z < c:
            scale[z], shift[z] = 1e-3, -1.0
    return scale, shift


def make_params(seed=5):
    """host tensors: w [64, 10], scale / shift [64] of the one-layer reader; w1 [32, 10], w2 [64, 64], ss1 [64], ss2 [128] of the
    two-layer reader; abd2 [192] in a training-style set (b, d non-zero) and the eval-style set (gamma * invstd, 0, 0)"""
    g = torch.Generator().manual_seed(seed)
    uni = lambda *s: torch.rand(*s, generator=g) * 2.0 - 1.0
    w = uni(C, F) * 0.3 / math.sqrt(F)
    scale, shift = _scale_shift(C, g)
    w1 = uni(C1, F) * 0.3 / math.sqrt(F)
    w2 = uni(C, C) / math.sqrt(C)
    sc1, sh1 = _scale_shift(C1, g)
    sc2, sh2 = _scale_shift(C, g)
    a2 = torch.rand(C, generator=g) + 0.5
    abd_train = torch.cat([a2, torch.randn(C, generator=g) * 0.01, torch.randn(C, generator=g) * 0.05])
    abd_eval = torch.cat([a2, torch.zeros(2 * C)])
    return types.SimpleNamespace(w=w, scale=scale, shift=shift, w1=w1, w2=w2, ss1=torch.cat([sc1, sh1]), ss2=torch.cat([sc2, sh2]),
                                 abd2={"train": abd_train, "eval": abd_eval})


def params_to(prm, device):
    out = types.SimpleNamespace(**{k: v.to(device) for k, v in vars(prm).items() if k != "abd2"})
    out.abd2 = {k: v.to(device) for k, v in prm.abd2.items()}
    return out


def make_grad(case, seed, device):
    """the test's own output gradient [P, 64]: about a third of it zero (relu'(out) = 0 applied by the caller)"""
    g = torch.Generator().manual_seed(seed)
    go = torch.randn(case.P, C, generator=g)
    return (go * (torch.rand(case.P, C, generator=g) > 0.3)).to(device)


def make_arg(case, kind, ref_arg, seed=11):
    """the argmax handed to a backward entry.  valid: the float64 first maximum; n: the first empty slot where there is one; above_n: a
    later empty slot where there is one; last: T - 1 everywhere (empty wherever n < T); zero: 0 everywhere"""
    t = case.T
    n = case.num.clamp(0, t).long()[:, None].expand(-1, C)
    if kind == "valid":
        return ref_arg.to(torch.uint8)
    if kind == "zero":
        return torch.zeros_like(ref_arg, dtype=torch.uint8)
    if kind == "last":
        return torch.full_like(ref_arg, t - 1, dtype=torch.uint8)
    if kind == "n":
        return torch.where(n < t, n, ref_arg).to(torch.uint8)
    assert kind == "above_n"
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(case.P, C, generator=g).to(n.device)
    above = n + 1 + (r * (t - 1 - n).clamp_min(0)).long()
    return torch.where(n + 1 < t, above.clamp_max(t - 1), ref_arg).to(torch.uint8)


# ---- float64 restatements -----------------------------------------------------------------------------------------------------------
def _slots(case):
    t = case.T
    n = case.num.clamp(0, t).long()
    ar = torch.arange(t, device=case.vox.device)
    valid = ar[None, :] < n[:, None]
    part = ar[None, :] <= n[:, None]     # the slots that take part in a maximum: the valid ones and the first empty one
    return n, valid, part


def decorate64(case):
    """-> f, the bound e(f) and the magnitudes |f|mag, each [P, T, 10] float64 with empty slots at zero"""
    t = case.T
    vx, vy, xo, yo = case.geo
    v = case.vox.double()
    n, valid, _ = _slots(case)
    nd = n.double().clamp_min(1.0)[:, None]       # n = 0: no valid slot, the mean is not used
    mean = v[:, :, :3].sum(1) / nd
    meanmag = v[:, :, :3].abs().sum(1) / nd
    cx, cy = case.coors[:, 3].double() * vx + xo, case.coors[:, 2].double() * vy + yo
    cxm, cym = (case.coors[:, 3].double() * vx).abs() + abs(xo), (case.coors[:, 2].double() * vy).abs() + abs(yo)
    centre, centremag = torch.stack([cx, cy], 1), torch.stack([cxm, cym], 1)
    m = valid[:, :, None].double()
    f = torch.cat([v, v[:, :, :3] - mean[:, None], v[:, :, :2] - centre[:, None]], 2) * m
    fmag = torch.cat([v.abs(), v[:, :, :3].abs() + meanmag[:, None], v[:, :, :2].abs() + centremag[:, None]], 2) * m
    chain = torch.tensor([0.0] * 5 + [t + 1.0] * 3 + [3.0] * 2, dtype=torch.float64, device=v.device)
    return f, gamma(chain) * fmag, fmag


def _linear(x, ex, xmag, w, k):
    """y = W x with k fma from zero -> (y, e(y), |y|mag)"""
    w = w.double()
    y, pe, ymag = x @ w.t(), ex @ w.abs().t(), xmag @ w.abs().t()
    return y, pe + gamma(k) * (ymag + pe), ymag


def _bn_relu(h, eh, hmag, scale, shift, valid=None, esc=0.0, esh=0.0):
    """y = relu(h scale + shift) by one fma -> (z, y, e(y)); with `valid`, the other slots hold relu(shift) without a rounding.
    esc / esh: how far the scale / shift the kernel received may lie from the float64 ones given here (0 when the test owns them)"""
    sc, sh = scale.double(), shift.double()
    z = h * sc + sh
    ez = sc.abs() * eh + (h.abs() + eh) * esc + esh + gamma(1) * ((sc.abs() + esc) * (hmag + eh) + sh.abs() + esh)
    if valid is not None:
        ez = torch.where(valid[:, :, None], ez, (torch.zeros_like(sh) + esh).expand_as(ez))
    return z, z.clamp_min(0.0), ez


def _prod(amag, ea, bmag, eb):
    return ea * bmag + amag * eb + ea * eb


def _sum_bound(e, mag, chain):
    return e + gamma(chain) * (mag + e)


def by_block(x, blocks):
    """[P, ...] -> [blocks, ...]: block b, wave w owns p = 4 b + w + k * 4 * blocks"""
    p, g = x.shape[0], 4 * blocks
    k = ceil_div(p, g)
    if k * g != p:
        x = torch.cat([x, x.new_zeros((k * g - p,) + tuple(x.shape[1:]))])
    return x.view((k, blocks, 4) + tuple(x.shape[1:])).sum((0, 2))


def by_wave(x, waves=BWD2_ROWS):
    """[P, ...] -> [waves, ...]: wave v owns p = v + k * waves"""
    p = x.shape[0]
    k = ceil_div(p, waves)
    if k * waves != p:
        x = torch.cat([x, x.new_zeros((k * waves - p,) + tuple(x.shape[1:]))])
    return x.view((k, waves) + tuple(x.shape[1:])).sum(0)


def first_max(y, part):
    """-> (max, its first slot, the gap to the runner-up) over the slots `part` of y [P, T, c]"""
    t = y.shape[1]
    ym = torch.where(part[:, :, None], y, torch.full_like(y, -math.inf))
    top = ym.amax(1)
    ar = torch.arange(t, device=y.device)[None, :, None]
    first = torch.where(ym == top[:, None], ar, t).amin(1)
    rest = torch.where(ar == first[:, None], torch.full_like(ym, -math.inf), ym).amax(1)
    return top, first, top - rest      # a single slot: the gap is inf


class Ref1:
    """the one-layer reader in float64"""

    def __init__(self, case, prm):
        self.case, self.prm = case, prm
        self.n, self.valid, self.part = _slots(case)
        self.f, self.ef, self.fmag = decorate64(case)
        self.h, self.eh, self.hmag = _linear(self.f, self.ef, self.fmag, prm.w, F)
        self.trips = ceil_div(case.P, 4 * blocks_mirror(case.P))

    def stats(self, blocks):
        """-> (slabs [blocks, 2, 64], their bounds)"""
        chain = self.trips * self.case.T + 2
        h, eh, hm = self.h, self.eh, self.hmag
        ref = torch.stack([by_block(h.sum(1), blocks), by_block((h * h).sum(1), blocks)], 1)
        e = torch.stack([by_block(eh.sum(1), blocks), by_block(_prod(h.abs(), eh, h.abs(), eh).sum(1), blocks)], 1)
        mag = torch.stack([by_block(hm.sum(1), blocks), by_block((hm * hm).sum(1), blocks)], 1)
        return ref, _sum_bound(e, mag, chain)

    def apply(self):
        """-> (y [P, T, 64], e(y)) with the empty slots at relu(shift)"""
        self.z, y, ey = _bn_relu(self.h, self.eh, self.hmag, self.prm.scale, self.prm.shift, self.valid, getattr(self.prm, "e_scale", 0.0),
                                 getattr(self.prm, "e_shift", 0.0))
        return y, ey

    def bwd(self, arg, g, blocks, e_g=None):
        """-> (rows [blocks, BWD_COLS], their bounds) for the test's own arg [P, 64] and g [P, 64]; e_g: how far the g the kernel
        received may lie from the float64 one given here"""
        t = self.case.T
        ar = torch.arange(t, device=g.device)[None, :, None]
        hot = ((ar == arg.long()[:, None]) & self.valid[:, :, None]).double()      # an empty slot: h = 0, f = 0
        gr = hot * g.double()[:, None]
        ga = gr.abs()
        ein = lambda a, b: torch.einsum("ptc,ptk->pkc", a, b).reshape(a.shape[0], -1)
        eg = torch.zeros_like(g, dtype=torch.float64) if e_g is None else e_g
        egr = hot * eg[:, None]
        light, heavy = self.trips + 2, self.trips * t + 2
        parts = [   # (per-pillar value, propagated error, magnitude, chain)
            (g.double(), eg, g.double().abs(), light),
            ((gr * self.h).sum(1), (ga * self.eh + egr * (self.hmag + self.eh)).sum(1), (ga * self.hmag).sum(1), light),
            (ein(gr, self.f), ein(ga, self.ef) + ein(egr, self.fmag + self.ef), ein(ga, self.fmag), light),
            (ein(self.h, self.f), ein(self.eh, self.fmag) + ein(self.hmag + self.eh, self.ef), ein(self.hmag, self.fmag), heavy),
            (self.f.sum(1), self.ef.sum(1), self.fmag.sum(1), heavy),
        ]
        ref = torch.cat([by_block(v, blocks) for v, _, _, _ in parts], 1)
        bound = torch.cat([_sum_bound(by_block(e, blocks), by_block(m, blocks), ch) for _, e, m, ch in parts], 1)
        return ref, bound


class Ref2:
    """the two-layer reader in float64"""

    def __init__(self, case, prm, defer=False):
        self.case, self.prm = case, prm
        self.n, self.valid, self.part = _slots(case)
        self.f, self.ef, self.fmag = decorate64(case)
        self.h1, self.eh1, self.h1mag = _linear(self.f, self.ef, self.fmag, prm.w1, F)
        self.trips = ceil_div(case.P, 4 * blocks_mirror(case.P))
        self.trips2 = ceil_div(case.P, BWD2_ROWS)
        if not defer:
            self.layer2()

    def layer2(self):
        """everything behind the first batch norm, from prm.ss1 (and prm.e_ss1, how far the kernel's copy may lie from it)"""
        prm = self.prm
        e1 = getattr(prm, "e_ss1", None)
        esc, esh = (0.0, 0.0) if e1 is None else (e1[:C1], e1[C1:])
        self.z1, self.x1, self.ex1 = _bn_relu(self.h1, self.eh1, self.h1mag, prm.ss1[:C1], prm.ss1[C1:], self.valid, esc, esh)
        self.m1, self.arg1, self.gap1 = first_max(self.x1, self.part)
        self.em1 = (self.ex1 * self.part[:, :, None]).amax(1)
        a, b = prm.w2[:, :C1].double(), prm.w2[:, C1:].double()
        self.A, self.B = a, b
        pe = self.ex1 @ a.abs().t() + (self.em1 @ b.abs().t())[:, None]
        self.h2 = self.x1 @ a.t() + (self.m1 @ b.t())[:, None]
        self.h2mag = self.x1 @ a.abs().t() + (self.m1 @ b.abs().t())[:, None]
        self.eh2 = pe + gamma(C) * (self.h2mag + pe)

    def tau(self):
        return TAU_REL * float(self.z1[self.valid].abs().max()) if bool(self.valid.any()) else 0.0

    def rejected(self):
        """[P] bool: pillars whose layer-1 gate or layer-1 argmax pfn2_bwd could decide differently in fp32"""
        tau = self.tau()
        gate = ((self.z1.abs() < tau) & self.valid[:, :, None]).any(2).any(1)
        tie = ((self.gap1 > 0) & (self.gap1 < tau)).any(1)
        return gate | tie

    def stats1(self, blocks):
        chain = self.trips * ceil_div(self.case.T, 2) + 3
        h, eh, hm = self.h1, self.eh1, self.h1mag
        dup = lambda x: torch.cat([x, x], -1)     # columns 32..63 duplicate 0..31
        ref = torch.stack([by_block(dup(h.sum(1)), blocks), by_block(dup((h * h).sum(1)), blocks)], 1)
        e = torch.stack([by_block(dup(eh.sum(1)), blocks), by_block(dup(_prod(h.abs(), eh, h.abs(), eh).sum(1)), blocks)], 1)
        mag = torch.stack([by_block(dup(hm.sum(1)), blocks), by_block(dup((hm * hm).sum(1)), blocks)], 1)
        return ref, _sum_bound(e, mag, chain)

    def stats2(self, blocks):
        """all T rows of every pillar: the empty row counts T - n times"""
        chain = self.trips * self.case.T + 2
        h, eh, hm = self.h2, self.eh2, self.h2mag
        ref = torch.stack([by_block(h.sum(1), blocks), by_block((h * h).sum(1), blocks)], 1)
        e = torch.stack([by_block(eh.sum(1), blocks), by_block(_prod(h.abs(), eh, h.abs(), eh).sum(1), blocks)], 1)
        mag = torch.stack([by_block(hm.sum(1), blocks), by_block((hm * hm).sum(1), blocks)], 1)
        return ref, torch.stack([_sum_bound(e[:, 0], mag[:, 0], chain), _sum_bound(e[:, 1], mag[:, 1], chain + 1)], 1)

    def apply(self):
        e2 = getattr(self.prm, "e_ss2", None)
        esc, esh = (0.0, 0.0) if e2 is None else (e2[:C], e2[C:])
        self.z2, y, ey = _bn_relu(self.h2, self.eh2, self.h2mag, self.prm.ss2[:C], self.prm.ss2[C:], None, esc, esh)
        return y, ey

    def bwd(self, arg2, gout, abd2, e_abd2=None, e_gout=None):
        """-> (rows [1024, BWD2_COLS], their bounds) for the test's own arg2, gout and abd2 (scale_shift1 is prm.ss1); e_abd2 / e_gout: how
        far the abd2 / gout the kernel received may lie from the float64 ones given here"""
        t, p = self.case.T, self.case.P
        dev = gout.device
        a2, b2, d2 = (abd2[i * C:(i + 1) * C].double() for i in range(3))
        ea2, eb2, ed2 = (0.0, 0.0, 0.0) if e_abd2 is None else (e_abd2[i * C:(i + 1) * C] for i in range(3))
        ar = torch.arange(t, device=dev)[None, :, None]
        hot = (ar == arg2.long()[:, None]).double()
        ga = hot * (a2 * gout.double())[:, None]      # arg2 >= n scatters to an empty slot: same z
        dh2 = ga + b2 * self.h2 + d2
        dh2mag = ga.abs() + b2.abs() * self.h2mag + d2.abs()
        eg = 0.0 if e_gout is None else e_gout
        pe = b2.abs() * self.eh2 + eb2 * (self.h2mag + self.eh2) + ed2 + hot * (ea2 * (gout.double().abs() + eg) + a2.abs() * eg)[:, None]
        edh2 = pe + gamma(3) * (dh2mag + pe)
        x1, ex1, m1, em1 = self.x1, self.ex1, self.m1, self.em1
        # dW2[:, :32] = sum dh2 (x) x1 per wave, dW2[:, 32:] = sum (sum_t dh2) (x) m1
        k = self.trips2
        pad = lambda x: torch.cat([x, x.new_zeros((k * BWD2_ROWS - p,) + tuple(x.shape[1:]))]).view((k, BWD2_ROWS) + tuple(x.shape[1:]))
        ein = lambda u, v: torch.einsum("kvtl,kvtj->vlj", pad(u), pad(v))
        dwa, dwa_mag = ein(dh2, x1), ein(dh2mag, x1)
        dwa_e = ein(edh2, x1 + ex1) + ein(dh2mag, ex1)
        sdh2, sdh2mag = dh2.sum(1), dh2mag.sum(1)
        esdh2 = _sum_bound(edh2.sum(1), sdh2mag, t)
        outer = lambda u, v: by_wave(u[:, :, None] * v[:, None, :])
        dwb, dwb_mag = outer(sdh2, m1), outer(sdh2mag, m1)
        dwb_e = outer(esdh2, m1 + em1) + outer(sdh2mag, em1)
        dw2 = torch.cat([dwa, dwb], 2).reshape(BWD2_ROWS, C * C)
        dw2_bound = torch.cat([_sum_bound(dwa_e, dwa_mag, k * t), _sum_bound(dwb_e, dwb_mag, k)], 2).reshape(BWD2_ROWS, C * C)
        # dz = W2^T dh2, g1 through max-1 / relu
        aa, ba = self.A.abs(), self.B.abs()
        dm1, dm1mag = sdh2 @ self.B, sdh2mag @ ba
        edm1 = _sum_bound(esdh2 @ ba, dm1mag, C)
        dz, dzmag = dh2 @ self.A, dh2mag @ aa
        edz = _sum_bound(edh2 @ aa, dzmag, C)
        oh1 = (ar == self.arg1[:, None]).double()
        gin = dz + oh1 * dm1[:, None]
        ginmag = dzmag + oh1 * dm1mag[:, None]
        egin = _sum_bound(edz + oh1 * edm1[:, None], ginmag, 1)
        gate = (self.z1 > 0).double()      # an empty slot: z1 = shift1
        g1, eg1, g1mag = gin * gate, egin * gate, ginmag * gate
        # decisions the kernel may take differently (none after screened_case(): tau > 2 max e(x1)): a gate whose pre-activation lies
        # within its own bound of zero lets gin through or not; a slot within the bounds of the layer-1 maximum (exact float64 ties
        # apart: the first slot wins in either precision) may receive dm1 instead of the float64 first maximum
        open_gate = ((self.z1.abs() <= ex1) & (ex1 > 0)).double()
        near = self.part[:, :, None] & (x1 < m1[:, None]) & (x1 >= m1[:, None] - (ex1 + em1[:, None]))
        moved = (near | ((oh1 > 0) & near.any(1)[:, None])).double()
        eg1 = eg1 + open_gate * (ginmag + egin) + moved * (dm1mag + edm1)[:, None]
        ein1 = lambda u, v: torch.einsum("ptc,ptk->pkc", u, v)
        wide = lambda x: torch.cat([x, torch.zeros_like(x)], -1).reshape(x.shape[0], -1)      # columns 32..63 are zero
        chain = k * ceil_div(t, 2) + 1
        h1, eh1, h1m, f, ef, fm = self.h1, self.eh1, self.h1mag, self.f, self.ef, self.fmag
        parts = [
            (wide(g1.sum(1)), wide(eg1.sum(1)), wide(g1mag.sum(1))),
            (wide((g1 * h1).sum(1)), wide(_prod(g1mag, eg1, h1m, eh1).sum(1)), wide((g1mag * h1m).sum(1))),
            (wide(ein1(g1, f)), wide(ein1(eg1, fm) + ein1(g1mag + eg1, ef)), wide(ein1(g1mag, fm))),
            (wide(ein1(h1, f)), wide(ein1(eh1, fm) + ein1(h1m + eh1, ef)), wide(ein1(h1m, fm))),
            (f.sum(1), ef.sum(1), fm.sum(1)),
        ]
        ref = torch.cat([dw2] + [by_wave(v) for v, _, _ in parts], 1)
        bound = torch.cat([dw2_bound] + [_sum_bound(by_wave(e), by_wave(m), chain) for _, e, m in parts], 1)
        return ref, bound


def screened_case(pillars, slots, prm, device="cpu"):
    """make_case, then redraw the pillars Ref2.rejected() names until none is left -> the host case; .rounds and .first_reject record
    the loop (a case that needs no redraw has rounds = 1: one screening)"""
    case = make_case(pillars, slots)
    prm_d = params_to(prm, device)
    for rnd in range(1, REDRAW_ROUNDS + 1):
        ref = Ref2(case_to(case, device), prm_d)
        bad = ref.rejected().cpu()
        if rnd == 1:
            case.first_reject = float(bad.double().mean())
        if not bool(bad.any()):
            assert ref.tau() > 2.0 * float(ref.ex1.max()), "the decision margin does not cover the fp32 error of x1"
            case.rounds = rnd
            return case
        _draw_points(case, bad.nonzero().flatten(), case.gen)
    raise AssertionError(f"P = {pillars}, T = {slots}: pillars left to redraw after {REDRAW_ROUNDS} rounds")


# ---- checkers -------------------------------------------------------------------------------------------------------------------------
def check_rows(got, ref, bound, what, family, names="row, column"):
    """every element of a slab / row list within its bound; a NaN is a miss"""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        idx = bad.nonzero()[:8].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first ({names}): {idx}, |err| / bound "
                             f"{[float(err[tuple(i)] / bound[tuple(i)]) if bound[tuple(i)] > 0 else math.inf for i in idx]}")
    _note(family, err, bound)


def bwd_sections(cols):
    """column ranges of a backward row, for the per-family report"""
    base = cols - BWD_COLS
    names = (("sum g", 0, C), ("sum g h", C, 2 * C), ("M1", 2 * C, (2 + F) * C), ("M2", (2 + F) * C, (2 + 2 * F) * C), ("M3", (2 + 2 * F) * C, BWD_COLS))
    out = [("dW2", 0, base)] if base else []
    return out + [(n, base + lo, base + hi) for n, lo, hi in names]


def check_bwd_rows(got, ref, bound, what, family):
    for name, lo, hi in bwd_sections(ref.shape[1]):
        check_rows(got[:, lo:hi], ref[:, lo:hi], bound[:, lo:hi], f"{what}, {name}", f"{family} {name}", "row, column of the section")


def check_argmax(y, ey, part, out, arg, what, family, h2=None, eh2=None, h2max=None):
    """out / arg (and h2_at_max) of an apply_max entry against y [P, T, 64] with bounds ey -> the share of pairs under the strict rule"""
    t = y.shape[1]
    top, first, gap = first_max(y, part)
    e_max = torch.where(part[:, :, None], ey, torch.zeros_like(ey)).amax(1)
    check_rows(out, top, e_max, f"{what}: out", f"{family} out", "pillar, channel")
    a = arg.long()
    assert bool((a < t).all()), f"{what}: arg holds a slot >= T = {t}"
    takes_part = torch.gather(part[:, :, None].expand(-1, -1, C), 1, a[:, None])[:, 0]
    assert bool(takes_part.all()), f"{what}: arg names a slot above the first empty one at {int((~takes_part).sum())} pairs"
    y_at, e_at = torch.gather(y, 1, a[:, None])[:, 0], torch.gather(ey, 1, a[:, None])[:, 0]
    # "y_ref[arg] >= max y_ref - bound" with bound = e[arg] + e_max, and the strict rule above a gap of 2 e_max: the kernel took arg
    # because ITS y[arg] >= ITS y[t*] (t* = the float64 maximum), so y_ref[arg] + e[arg] >= y[arg] >= y[t*] >= y_ref[t*] - e[t*] and
    # e[t*] <= e_max.  A single e_max would reject a correct kernel whose two values both sit at their bounds
    bad = ~(y_at >= top - (e_at + e_max))
    assert not bool(bad.any()), f"{what}: arg is not a maximum at {int(bad.sum())} pairs; first (pillar, channel): {bad.nonzero()[:8].tolist()}"
    strict = (gap == 0) | (gap > 2.0 * e_max)
    wrong = strict & (a != first)
    assert not bool(wrong.any()), (f"{what}: arg is not the FIRST maximum at {int(wrong.sum())} pairs that float64 decides; first (pillar, channel, "
                                   f"arg, float64): {[(i, j, int(a[i, j]), int(first[i, j])) for i, j in wrong.nonzero()[:8].tolist()]}")
    share = float(strict.double().mean())
    assert share >= STRICT_SHARE, f"{what}: only {share:.3f} of the pairs fall under the strict first-maximum rule"
    if h2max is not None:
        check_rows(h2max, torch.gather(h2, 1, a[:, None])[:, 0], torch.gather(eh2, 1, a[:, None])[:, 0], f"{what}: h2_at_max", f"{family} h2_at_max",
                   "pillar, channel")
    return share


# ---- fp32 host emulation (what the CPU checks feed the checkers); each function takes a `defect` switch --------------------------------
DEFECTS = ("skip_last_of_second_trip", "pillar_dealt_twice", "empty_multiplicity_minus_1", "empty_row_left_out", "last_maximum", "m3_zero",
           "upper_columns_not_zeroed", "column_counted_twice", "idle_row_unwritten", "num_not_clamped", "centre_x_from_y")


def _emu_feats(case, defect):
    t = case.T
    vx, vy, xo, yo = case.geo
    v = case.vox.float()
    n = case.num.clamp_min(0) if defect == "num_not_clamped" else case.num.clamp(0, t)
    valid = torch.arange(t, device=v.device)[None, :] < n[:, None]
    mean = v[:, :, :3].sum(1) / n.float().clamp_min(1.0)[:, None]
    cx = case.coors[:, 2 if defect == "centre_x_from_y" else 3].float() * vx + xo
    cy = case.coors[:, 2].float() * vy + yo
    f = torch.cat([v, v[:, :, :3] - mean[:, None], v[:, :, 0:1] - cx[:, None, None], v[:, :, 1:2] - cy[:, None, None]], 2)
    return f * valid[:, :, None].float(), case.num.clamp(0, t).long(), valid


def _emu_group(x, group, per_trip, owner, defect):
    """per-pillar rows x [P, cols] -> group(x) with the dealing defects"""
    p = x.shape[0]
    x = x.clone()
    if defect == "skip_last_of_second_trip" and p > per_trip:
        x[min(p, 2 * per_trip) - 1] = 0.0
    out = group(x)
    if defect == "pillar_dealt_twice" and p > 1:
        out[owner(0)] += x[1]
    return out


def _emu_blocks(x, blocks, defect):
    return _emu_group(x, lambda v: by_block(v, blocks), 4 * blocks, lambda p: (p % (4 * blocks)) // 4, defect)


def _emu_max(y, part, defect):
    t = y.shape[1]
    ym = torch.where(part[:, :, None], y, torch.full_like(y, -math.inf))
    top = ym.amax(1)
    ar = torch.arange(t, device=y.device)[None, :, None]
    hit = ym == top[:, None]
    arg = torch.where(hit, ar, -1).amax(1) if defect == "last_maximum" else torch.where(hit, ar, t).amin(1)
    return top, arg


def _emu_unwritten(case, blocks_x4, defect, *outs):
    if defect == "skip_last_of_second_trip" and case.P > blocks_x4:
        for o in outs:
            o[min(case.P, 2 * blocks_x4) - 1] = float("nan") if o.dtype.is_floating_point else 0xEE


def emu_stats(case, prm, blocks, defect=None):
    f, _, _ = _emu_feats(case, defect)
    h = f @ prm.w.float().t()
    return _emu_blocks(torch.cat([h.sum(1), (h * h).sum(1)], 1), blocks, defect).view(blocks, 2, C)


def emu_apply_max(case, prm, defect=None):
    f, n, valid = _emu_feats(case, defect)
    y = (f @ prm.w.float().t() * prm.scale + prm.shift).clamp_min(0.0)
    y = torch.where(valid[:, :, None], y, prm.shift.clamp_min(0.0).expand_as(y))
    out, arg = _emu_max(y, _slots(case)[2], defect)
    arg = arg.to(torch.uint8)
    _emu_unwritten(case, 4 * blocks_mirror(case.P), defect, out, arg)
    return out, arg


def _emu_bwd_parts(f, h, gr, g_sum, defect):
    ein = lambda a, b: torch.einsum("ptc,ptk->pkc", a, b)      # [P, 10, c]
    m3 = f.sum(1)
    if defect == "m3_zero":
        m3 = torch.zeros_like(m3)
    return [g_sum, (gr * h).sum(1), ein(gr, f), ein(h, f), m3]


def emu_bwd(case, prm, arg, g, blocks, defect=None):
    f, n, valid = _emu_feats(case, defect)
    h = f @ prm.w.float().t()
    ar = torch.arange(case.T, device=g.device)[None, :, None]
    gr = ((ar == arg.long()[:, None]) & valid[:, :, None]).float() * g[:, None]
    return _emu_blocks(torch.cat([x.reshape(case.P, -1) for x in _emu_bwd_parts(f, h, gr, g, defect)], 1), blocks, defect)


def _emu_layer1(case, prm, defect):
    f, n, valid = _emu_feats(case, defect)
    h1 = f @ prm.w1.float().t()
    sc1, sh1 = prm.ss1[:C1], prm.ss1[C1:]
    z1 = h1 * sc1 + sh1
    x1 = torch.where(valid[:, :, None], z1.clamp_min(0.0), sh1.clamp_min(0.0).expand_as(z1))
    part = _slots(case)[2]
    m1, arg1 = _emu_max(x1, part, None)
    h2 = x1 @ prm.w2[:, :C1].float().t() + (m1 @ prm.w2[:, C1:].float().t())[:, None]
    return f, n, valid, part, h1, z1, x1, m1, arg1, h2


def emu_stats1(case, prm, blocks, defect=None):
    f, _, _ = _emu_feats(case, defect)
    h = f @ prm.w1.float().t()
    s = torch.cat([h.sum(1), h.sum(1), (h * h).sum(1), (h * h).sum(1)], 1)
    return _emu_blocks(s, blocks, defect).view(blocks, 2, C)


def _emu_mult(case, n, valid, defect):
    """the weight of every slot in a sum over all T rows: the empty row counts T - n times (kept on the first empty slot)"""
    t = case.T
    first_empty = torch.arange(t, device=n.device)[None, :] == n[:, None]
    count = (t - n).float()
    if defect == "empty_multiplicity_minus_1":
        count = count - 1.0
    if defect == "empty_row_left_out":
        count = torch.zeros_like(count)
    return valid.float() + first_empty.float() * count[:, None]


def emu_stats2(case, prm, blocks, defect=None):
    f, n, valid, part, h1, z1, x1, m1, arg1, h2 = _emu_layer1(case, prm, defect)
    mult = _emu_mult(case, n, valid, defect)[:, :, None]
    return _emu_blocks(torch.cat([(mult * h2).sum(1), (mult * h2 * h2).sum(1)], 1), blocks, defect).view(blocks, 2, C)


def emu_apply_max2(case, prm, defect=None):
    f, n, valid, part, h1, z1, x1, m1, arg1, h2 = _emu_layer1(case, prm, defect)
    y = (h2 * prm.ss2[:C] + prm.ss2[C:]).clamp_min(0.0)
    out, arg = _emu_max(y, part, defect)
    h2max = torch.gather(h2, 1, arg[:, None])[:, 0]
    arg = arg.to(torch.uint8)
    _emu_unwritten(case, 4 * blocks_mirror(case.P), defect, out, arg, h2max)
    return out, arg, h2max


def emu_bwd2(case, prm, arg2, gout, abd2, defect=None):
    f, n, valid, part, h1, z1, x1, m1, arg1, h2 = _emu_layer1(case, prm, defect)
    t, p = case.T, case.P
    a2, b2, d2 = (abd2[i * C:(i + 1) * C].float() for i in range(3))
    ar = torch.arange(t, device=gout.device)[None, :, None]
    # one row per pillar stands for its empty slots: the arg-2 gradient of any empty slot lands there, the b / d terms T - n times
    a = torch.minimum(arg2.long(), n[:, None])
    mult = _emu_mult(case, n, valid, defect)[:, :, None]
    dh2 = (ar == a[:, None]).float() * (a2 * gout)[:, None] + mult * (b2 * h2 + d2)
    z = torch.cat([x1, m1[:, None].expand(-1, t, -1)], 2)
    dw2 = torch.einsum("ptl,ptj->plj", dh2, z).reshape(p, C * C)
    dz = dh2 @ prm.w2.float()
    gin = dz[:, :, :C1] + (ar == arg1[:, None]).float() * dz[:, :, C1:].sum(1)[:, None]
    gate = torch.where(valid[:, :, None], z1 > 0, (prm.ss1[C1:] > 0).expand_as(z1))
    g1 = gin * gate.float() * part[:, :, None].float()
    upper = (lambda x: x) if defect == "upper_columns_not_zeroed" else torch.zeros_like
    wide = lambda x: torch.cat([x, upper(x)], -1).reshape(p, -1)
    parts = _emu_bwd_parts(f, h1, g1, g1.sum(1), defect)
    if defect == "column_counted_twice":
        parts[1][:, 5] *= 2.0
    rows = _emu_group(torch.cat([dw2] + [wide(x) for x in parts[:4]] + [parts[4]], 1), by_wave, BWD2_ROWS, lambda q: q % BWD2_ROWS, defect)
    if defect == "idle_row_unwritten":
        rows[BWD2_ROWS - 1] = float("nan")      # the last wave is idle whenever P < 1024
    return rows


# ---- the Python side on top of the entries (PillarFeatureNet through _FusedPfnFn / _FusedPfn2Fn) -----------------------------------------
# The module folds the slabs with torch (partial.sum(0): any order, at most rows - 1 roundings per element), finalises both batch norms
# with s2d_bn1d_finalize_fwd_f32 / _bwd_f32 and assembles dW = a M1 + b M2 + d M3 with three products and two additions.  The finalize
# outputs are bounded as in tests/bn_pass_ref.py: the float64 formula at the corners of the box its inputs may lie in, widened by
# 8 ulp_fp32 of the largest intermediate; those half-widths enter the kernels' bounds as e(scale), e(shift), e(a), e(b), e(d).
def fold(ref, bound):
    """torch's sum over the rows of a partial list -> (float64 sum, its bound)"""
    return ref.sum(0), _sum_bound(bound.sum(0), ref.abs().sum(0), max(ref.shape[0] - 1, 1))


def box(fn, args, deltas):
    """fn(*args) -> {name: (value, m)}; -> {name: (value at the centre, half-width over the corners of args +- deltas + 8 ulp_fp32(m))}"""
    import itertools
    import bn_pass_ref as B
    centre = fn(*args)
    half = {k: torch.zeros_like(v[0]) for k, v in centre.items()}
    for signs in itertools.product((-1.0, 1.0), repeat=len(args)):
        corner = fn(*[a + s * d for a, s, d in zip(args, signs, deltas)])
        for k in half:
            half[k] = torch.maximum(half[k], (corner[k][0] - centre[k][0]).abs())
    return {k: (centre[k][0], half[k] + 8.0 * B.ulp_fp32(centre[k][1])) for k in centre}


class ModuleRef:
    """PillarFeatureNet (one or two fused layers, train or eval) in float64 with propagated bounds.  layers: per PFN layer a namespace of
    the fp32 tensors w, gamma, beta, rm, rv (as they were BEFORE the forward) and the floats eps, momentum"""

    def __init__(self, case, layers, train):
        self.case, self.layers, self.train = case, layers, train
        self.rows = float(case.P * case.T)
        self.blocks = blocks_mirror(case.P)

    def _bn_fwd(self, lyr, stats):
        import bn_pass_ref as B
        g, b, rm, rv = lyr.gamma.double(), lyr.beta.double(), lyr.rm.double(), lyr.rv.double()
        if self.train:
            (s, ds) = stats()
            return box(lambda s0, s1: B.fwd_finalize(s0, s1, self.rows, g, b, lyr.eps, lyr.momentum, rm, rv), (s[0], s[1]), (ds[0], ds[1]))

        def fn():
            invstd = torch.rsqrt(rv + lyr.eps)
            scale = g * invstd
            m = B._big(rv + lyr.eps, invstd, scale)
            return {"mean": (rm, rm.abs()), "invstd": (invstd, m), "scale": (scale, m), "shift": (b - rm * scale, B._big(m, b, rm * scale))}
        return box(fn, (), ())

    def _bn_bwd(self, lyr, sg, dsg, sgx, dsgx, bn):
        import bn_pass_ref as B
        g = lyr.gamma.double()

        def fn(sg_, sgx_, mean, invstd):
            out = dict(B.bwd_finalize_local(sg_, sgx_, mean, invstd))
            if self.train:
                out.update(B.bwd_finalize_global(sg_, sgx_, self.rows, g, mean, invstd))
            else:
                a = g * invstd
                zero = torch.zeros_like(a)
                out.update({"a": (a, a.abs()), "b": (zero, zero), "d": (zero, zero)})
            return out
        fin = box(fn, (sg, sgx, bn["mean"][0], bn["invstd"][0]), (dsg, dsgx, bn["mean"][1], bn["invstd"][1]))
        if not self.train:      # the eval shortcut passes exact zeros
            fin["b"] = fin["d"] = (torch.zeros_like(sg), torch.zeros_like(sg))
        return fin

    def forward(self):
        """-> {name: (value, bound)} of the running statistics; sets self.y / self.ey, the last layer's outputs per slot"""
        case, lyr, blocks = self.case, self.layers, self.blocks
        res = {}
        if len(lyr) == 2:
            prm = types.SimpleNamespace(w1=lyr[0].w, w2=lyr[1].w)
            ref = Ref2(case, prm, defer=True)

            def stats1():
                s, ds = fold(*ref.stats1(blocks))
                return s[:, :C1], ds[:, :C1]      # the module's [:, :32] column selection
            bn1 = self._bn_fwd(lyr[0], stats1)
            prm.ss1, prm.e_ss1 = torch.cat([bn1["scale"][0], bn1["shift"][0]]), torch.cat([bn1["scale"][1], bn1["shift"][1]])
            ref.layer2()
            bn2 = self._bn_fwd(lyr[1], lambda: fold(*ref.stats2(blocks)))
            prm.ss2, prm.e_ss2 = torch.cat([bn2["scale"][0], bn2["shift"][0]]), torch.cat([bn2["scale"][1], bn2["shift"][1]])
            self.bn = [bn1, bn2]
        else:
            prm = types.SimpleNamespace(w=lyr[0].w)
            ref = Ref1(case, prm)
            bn = self._bn_fwd(lyr[0], lambda: fold(*ref.stats(blocks)))
            prm.scale, prm.shift, prm.e_scale, prm.e_shift = bn["scale"][0], bn["shift"][0], bn["scale"][1], bn["shift"][1]
            self.bn = [bn]
        self.ref, self.prm = ref, prm
        self.y, self.ey = ref.apply()
        if self.train:
            for i, bn in enumerate(self.bn):
                res[f"pfn_layers.{i}.norm.running_mean"], res[f"pfn_layers.{i}.norm.running_var"] = bn["running_mean"], bn["running_var"]
        return res

    def ambiguous(self):
        """-> ([P] bool: pillars to redraw, [32] bool: layer-1 channels whose shift lies within the margin of the ReLU's zero): the
        screening of pfn2_bwd (Ref2.rejected()) for the two-layer reader.  The one-layer backward recomputes no decision.  The gate of
        the last layer (out > 0 in the backward) is not screened: where out lies within its own bound of zero the bounds of the
        gradients carry both outcomes (_open_out), and so does every layer-1 decision that lies within its bound (Ref2.bwd)"""
        ref = self.ref
        return ref.rejected(), self.prm.ss1[C1:].abs() < ref.tau()

    def check_out(self, out, arg):
        """out against the float64 value at the kernel's own slot; the slot itself must be a maximum within the bounds"""
        a = arg.long()
        y_at, e_at = torch.gather(self.y, 1, a[:, None])[:, 0], torch.gather(self.ey, 1, a[:, None])[:, 0]
        check_rows(out, y_at, e_at, "module: out", "module out", "pillar, channel")
        part = self.ref.part
        top = torch.where(part[:, :, None], self.y, torch.full_like(self.y, -math.inf)).amax(1)
        e_max = torch.where(part[:, :, None], self.ey, torch.zeros_like(self.ey)).amax(1)
        assert bool(torch.gather(part[:, :, None].expand(-1, -1, C), 1, a[:, None]).all()), "module: arg names a slot above the first empty one"
        assert bool((y_at >= top - (e_at + e_max)).all()), "module: the saved arg is not a maximum"
        differs = (out > 0) != (y_at > 0)
        assert not bool((differs & ~self._open_out(a)).any()), "module: out > 0 decided differently than in float64 outside the bound of out"
        return y_at

    def _open_out(self, a):
        """[P, 64] bool: out lies within its own bound of the ReLU's zero - the backward's out > 0 may fall either way"""
        at = lambda x: torch.gather(x, 1, a[:, None])[:, 0]
        z = self.ref.z2 if len(self.layers) == 2 else self.ref.z
        return (at(z).abs() <= at(self.ey)) & (at(self.ey) > 0)

    def backward(self, arg, dout):
        """-> {parameter name: (gradient, bound)} for the kernel's saved arg and the test's dout"""
        import bn_pass_ref as B  # noqa: F401
        case, lyr, ref = self.case, self.layers, self.ref
        a = arg.long()
        at = lambda x: torch.gather(x, 1, a[:, None])[:, 0]
        go = dout.double() * (at(self.y) > 0).double()
        ego = dout.double().abs() * self._open_out(a).double()      # where out > 0 may fall either way, g is dout or 0
        res = {}

        def assemble(fin, m1, e1, m2, e2, m3, e3):
            """dW = a M1 + b M2 + d M3 (M1, M2 [c, 10], M3 [10]): three products, two additions"""
            terms = [(fin["a"], m1, e1), (fin["b"], m2, e2), (fin["d"], m3[None, :].expand_as(m1), e3[None, :].expand_as(m1))]
            val = sum(c[0][:, None] * m for c, m, _ in terms)
            err = sum(_prod(c[0].abs()[:, None], c[1][:, None], m.abs(), e) for c, m, e in terms)
            mag = sum(c[0].abs()[:, None] * m.abs() for c, m, _ in terms)
            return val, _sum_bound(err, mag, 3)

        if len(lyr) == 2:
            p = case.P
            sg, dsg = go.sum(0), _sum_bound(ego.sum(0), go.abs().sum(0), max(p - 1, 1))
            sgx = (go * at(ref.h2)).sum(0)
            dsgx = _sum_bound((go.abs() * at(ref.eh2) + ego * (at(ref.h2mag) + at(ref.eh2))).sum(0), (go.abs() * at(ref.h2mag)).sum(0), p)
            fin2 = self._bn_bwd(lyr[1], sg, dsg, sgx, dsgx, self.bn[1])
            res["pfn_layers.1.norm.weight"], res["pfn_layers.1.norm.bias"] = fin2["dgamma"], fin2["dbeta"]
            abd2, e_abd2 = torch.cat([fin2[k][0] for k in "abd"]), torch.cat([fin2[k][1] for k in "abd"])
            r, dr = fold(*ref.bwd(arg, go, abd2, e_abd2, ego))
            res["pfn_layers.1.linear.weight"] = (r[:C * C].view(C, C), dr[:C * C].view(C, C))
            r, dr, c = r[C * C:], dr[C * C:], C1
        else:
            r, dr, c = *fold(*ref.bwd(arg, go, self.blocks, ego)), C
        sec = lambda x, lo, hi: x[lo * C:hi * C].view(hi - lo, C)[:, :c]      # rows of 64 columns; the two-layer reader keeps [:, :32]
        fin = self._bn_bwd(lyr[0], sec(r, 0, 1)[0], sec(dr, 0, 1)[0], sec(r, 1, 2)[0], sec(dr, 1, 2)[0], self.bn[0])
        res["pfn_layers.0.norm.weight"], res["pfn_layers.0.norm.bias"] = fin["dgamma"], fin["dbeta"]
        m3lo = (2 + 2 * F) * C
        res["pfn_layers.0.linear.weight"] = assemble(fin, sec(r, 2, 2 + F).t(), sec(dr, 2, 2 + F).t(), sec(r, 2 + F, 2 + 2 * F).t(),
                                                     sec(dr, 2 + F, 2 + 2 * F).t(), r[m3lo:m3lo + F], dr[m3lo:m3lo + F])
        return res
