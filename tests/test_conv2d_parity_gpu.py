"""Exact parity of every dense 2-D tile kernel of csrc/conv2d_nhwc.hip at every tile plan, called through _lib.load() with raw pointers.
References, the plan mirror, the checkers and the reasoning behind them: tests/conv2d_ref.py; tests/test_conv2d_checks_cpu.py shows
that the checkers can fail.

Every case forces its plan with s2d_conv2d_debug_force (include/s2d_debug.h), asserts that the plan report s2d_conv2d_plan shows the
kernel family, BN, rows per tile and NS it meant to reach (and that the entry's own *_stats_tiles / *_tile_rows query agrees, asked
unmemoised through fn.__wrapped__), then launches twice into fresh NaN-filled, guarded outputs from an x that sits between NaN fences:
the two results are bit-equal, every element is written, every guard intact, y is torch.equal to the int64 reference and each
statistics slab to the int64 sums over its own tile's rows.  Outside the exact set: the rounding set (bit-equal to
round-to-nearest-even, bounded sum of squares) and the GELU backward sums (bounded).  The override is restored after every test.

test_case_tables_cover_every_instantiation asserts, on the tables alone, that every instantiation the launchers can select has a case.
"""
import collections
import ctypes
import functools

import pytest
import torch

import bn_pass_ref as R
import conv2d_ref as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
LINES = {}      # case-group tag -> a plan line (test_zz_report prints them: profiles/conv2d_parity.txt)
TOPS = {}       # case-group -> largest |ref|

ENTRY = {C.K3: "s2d_conv2d3x3_nhwc_bf16", C.K3_BNBWD: "s2d_conv2d3x3_nhwc_bf16_bnbwd", C.K1: "s2d_conv2d1x1_nhwc_bf16",
         C.K1_BNBWD: "s2d_conv2d1x1_nhwc_bf16_bnbwd", C.UP: "s2d_convup_nhwc_bf16", C.K4S2: "s2d_conv2d4x4s2_nhwc_bf16",
         C.K2S2: "s2d_conv2d2x2s2_nhwc_bf16"}


@functools.lru_cache(maxsize=None)
def L():
    from sparse2dense_amd import _lib
    return _lib.load()


def last_error():
    from sparse2dense_amd import _lib
    return _lib.last_error()


def raw(name):
    """the unmemoised query"""
    fn = getattr(L(), name)
    return getattr(fn, "__wrapped__", fn)


def force(bm=-1, ns=-1, shared_a=-1, k64=-1):
    assert L().s2d_conv2d_debug_force(bm, ns, shared_a, k64) == 0, last_error()


@pytest.fixture(autouse=True)
def _restore_plan():
    try:
        yield
    finally:
        force()


def plan_of(g):
    out = (ctypes.c_int32 * 8)()
    rc = L().s2d_conv2d_plan(g.kind, g.n, g.h, g.w, g.cin, g.cout, g.pad, g.stride, g.ks, out)
    return rc, C.Plan(*list(out))


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def zero_page():
    return torch.zeros(64, dtype=torch.uint8, device=DEV)


def pack(g, w):
    """the weight image the entry of g reads, from the float32 weight on the device"""
    wd = w.to(DEV).contiguous()
    out = torch.full((w.numel(),), float("nan"), dtype=C.BF, device=DEV)
    if g.kind in (C.K3, C.K3_BNBWD):
        rc = L().s2d_conv2d3x3_pack_weights_bf16(p(wd), g.cin, g.cout, 0, 0, p(out), stream())
    elif g.kind in (C.K1, C.K1_BNBWD):
        rc = L().s2d_conv2d1x1_pack_weights_bf16(p(wd), g.cin, g.cout, 0, p(out), stream())
    elif g.kind == C.UP:
        rc = L().s2d_convup_pack_weights_bf16(p(wd), g.cin, g.cout, g.ks, p(out), stream())
    elif g.kind == C.K4S2:
        rc = L().s2d_conv2d4x4s2_pack_weights_bf16(p(wd), g.cin, g.cout, p(out), stream())
    else:
        rc = L().s2d_conv2d2x2s2_pack_weights_bf16(p(wd), g.cin, g.cout, 0, p(out), stream())
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return out


def launch(g, x, packed, bias, y, slabs, bb=None):
    """one call of the entry of g with raw pointers -> its return code"""
    e, zp, s = getattr(L(), ENTRY[g.kind]), p(zero_page()), stream()
    if g.kind == C.K3:
        return e(p(x), p(packed), p(bias), zp, g.n, g.h, g.w, g.cin, g.cout, g.pad, g.stride, p(y), p(slabs), s)
    if g.kind == C.K3_BNBWD:
        z, scale, shift, act = bb
        return e(p(x), p(packed), zp, g.n, g.h, g.w, g.cin, g.cout, g.pad, p(y), p(z), p(scale), p(shift), act, p(slabs), s)
    if g.kind == C.K1:
        return e(p(x), p(packed), p(bias), zp, g.n, g.h, g.w, g.cin, g.cout, p(y), p(slabs), s)
    if g.kind == C.K1_BNBWD:
        z, scale, shift, act = bb
        return e(p(x), p(packed), zp, g.n, g.h, g.w, g.cin, g.cout, p(y), p(z), p(scale), p(shift), act, p(slabs), s)
    if g.kind == C.UP:
        return e(p(x), p(packed), p(bias), zp, g.n, g.h, g.w, g.cin, g.cout, g.ks, p(y), p(slabs), s)
    if g.kind == C.K4S2:
        return e(p(x), p(packed), zp, g.n, g.h, g.w, g.cin, g.cout, p(y), s)
    return e(p(x), p(packed), p(bias), zp, g.n, g.h, g.w, g.cin, g.cout, p(y), p(slabs), s)


def tiles_query(g):
    """the entry's own statistics-slab count (unmemoised), None where the entry has no such query"""
    if g.kind in (C.K3, C.K3_BNBWD):
        return raw("s2d_conv2d3x3_stats_tiles")(g.n, g.h, g.w, g.cin, g.cout, g.pad, g.stride)
    if g.kind in (C.K1, C.K1_BNBWD):
        return raw("s2d_conv2d1x1_stats_tiles")(g.n, g.h, g.w, g.cin, g.cout)
    if g.kind == C.UP:
        return raw("s2d_convup_stats_tiles")(g.n, g.h, g.w, g.cin, g.cout, g.ks)
    if g.kind == C.K2S2:
        return raw("s2d_conv2d2x2s2_stats_tiles")(g.n, g.h, g.w)
    return None


@functools.lru_cache(maxsize=None)
def operands(g, amp, seed, bias):
    """operands and the int64 reference, computed once per (geometry, amplitude, seed, bias) and shared by every plan that runs them"""
    ref_g = g._replace(kind={C.K3_BNBWD: C.K3, C.K1_BNBWD: C.K1}.get(g.kind, g.kind))
    x, w, b = C.int_operands(ref_g, amp, seed, bias)
    ref = C.reference(ref_g, x, w, b)
    return C.nhwc_rows(x), w, b, ref


Case = collections.namedtuple("Case", "group tag g force expect mode bias stats act seed")


def run_case(c):
    g = c.g
    force(*c.force)
    rc, plan = plan_of(g)
    assert rc == 0, last_error()
    assert (plan.family, plan.bn, plan.rows, plan.ns) == c.expect, f"{c.tag}: the plan report {plan} is not the plan this case is for {c.expect}"
    m = C.gemm_rows(g)
    row_tiles = C.ceil_div(m, plan.rows)
    assert (plan.gx, plan.gy, plan.gz) == (C.ceil_div(row_tiles, 8) * 8, g.cout // plan.bn, 4 if g.kind == C.UP else 1), plan
    assert plan.tiles == plan.gz * row_tiles
    tq = tiles_query(g)
    assert tq is None or tq == plan.tiles, (tq, plan)
    if g.kind in (C.K3, C.K3_BNBWD):
        assert raw("s2d_conv2d3x3_tile_rows")(g.n, g.h, g.w, g.cin, g.cout, g.pad, g.stride) == plan.rows
    xrows, w, b, ref = operands(g, 1 if c.mode == "exact" else 3, c.seed, c.bias)
    top = int(ref.abs().max())
    TOPS[c.group] = max(TOPS.get(c.group, 0), top)
    LINES.setdefault((c.group, c.expect), C.plan_line(c.tag, g, plan))
    packed = pack(g, w)
    xbuf, x = C.fenced(xrows, C.fence_rows(g), C.BF, DEV)
    bias = None if b is None else b.to(DEV)
    bb_host = bb = None
    if c.act is not None:
        z, scale, shift = C.bnbwd_operands(m, g.cout, c.seed + 1)
        bb_host = (z, scale, shift, c.act)
        zbuf, zd = C.fenced(z, 2, C.BF, DEV)
        bb = (zd, scale.to(DEV), shift.to(DEV), c.act)
    outs = []
    for _ in range(2):
        ybuf, y = R.poisoned(C.out_pixels(g), g.cout, dtype=C.BF, device=DEV)
        slabbuf, slabs = R.poisoned(plan.tiles, 2, g.cout, dtype=F32, device=DEV) if c.stats else (None, None)
        rc = launch(g, x, packed, bias, y, slabs, bb)
        assert rc == 0, (c.tag, last_error())
        torch.cuda.synchronize()
        outs.append((ybuf, slabbuf))
    R.check_bits(outs[0][0], outs[1][0], c.tag + ": y of the two launches", "row, channel")
    if c.stats:
        R.check_bits(outs[0][1], outs[1][1], c.tag + ": slabs of the two launches", "slab, which, channel")
    ybuf, slabbuf = outs[0]
    R.assert_written(ybuf, c.tag + " y")              # on the device: guards bit-intact, body finite
    C.check_case(g, plan, c.mode, ref, ybuf.cpu(), None if slabbuf is None else slabbuf.cpu(), bb_host, what=c.tag,
                 family="GELU backward sums" if c.act == 2 else ("rounding set, sum of squares" if c.mode == "rounded" else None))


# ---- case tables ------------------------------------------------------------------------------------------------------------------------
def pick_hw(m):
    """m = ho * wo with ho the largest divisor <= sqrt(m) (a prime gives the one-row image 1 x m)"""
    ho = max(d for d in range(1, int(m ** 0.5) + 1) if m % d == 0)
    return ho, m // ho


def geo_rows(kind, n, per_image, cin, cout, pad=1, stride=1, ks=None):
    """the entry arguments whose implicit GEMM has n * per_image rows"""
    ho, wo = pick_hw(per_image)
    if kind in (C.K3, C.K3_BNBWD):
        if stride == 1:
            h, w = ho + 2 - 2 * pad, wo + 2 - 2 * pad
        else:   # one odd and one even extent
            h, w = (2 * ho - 1, 2 * wo) if pad == 1 else (2 * ho + 1, 2 * wo + 2)
    elif kind == C.K4S2:
        h, w = 2 * ho, 2 * wo
    elif kind == C.K2S2:
        h, w = 2 * ho + 1, 2 * wo
    else:
        h, w = ho, wo
    g = C.geo(kind, n, h, w, cin, cout, pad, stride, ks)
    assert C.gemm_rows(g) == n * per_image, (g, n * per_image)
    return g


def row_edges(r):
    """(tag, images, GEMM rows per image) around a tile height r"""
    return [(f"m = {r} - 1", 1, r - 1), (f"m = {r}", 1, r), (f"m = {r} + 1", 1, r + 1), ("m = 7", 1, 7), ("tiles straddle 3 images", 3, 35),
            ("7 tiles", 1, 7 * r - 3), ("8 tiles", 1, 8 * r), ("9 tiles", 1, 8 * r + 1)]


COMBOS = [(True, True), (False, True), (True, False), (False, False)]   # (bias, statistics)
NO_BIAS = (C.K4S2, C.K3_BNBWD, C.K1_BNBWD)
K32_KINDS = [("3x3", C.K3, 64, None), ("1x1", C.K1, 128, None), ("up ks 3", C.UP, 128, 3), ("up ks 4", C.UP, 64, 4), ("4x4s2", C.K4S2, 64, None)]
CASES = []


def add(group, tag, g, frc, expect, mode="exact", combo=0, act=None, seed=0):
    bias, stats = COMBOS[combo % 4]
    if g.kind in NO_BIAS:
        bias = False
    if g.kind == C.K4S2:
        stats = False
    if act is not None:
        stats = True
    CASES.append(Case(group, f"{group}: {tag} [{C.KIND_NAMES[g.kind]} {g.n}x{g.h}x{g.w} {g.cin}->{g.cout} p{g.pad} s{g.stride} k{g.ks}]", g,
                      frc, expect, mode, bias, stats, act, seed))


def _build():
    # k32, rows 64 / 96 / 128 forced, every entry that has MI variants, row edges of that tile height
    for name, kind, cin, ks in K32_KINDS:
        for r in (64, 96, 128):
            for i, (tag, n, per) in enumerate(row_edges(r)):
                add(f"k32 {name} rows {r}", tag, geo_rows(kind, n, per, cin, 128, ks=ks), (r, 32, 0, 0), (C.K32, 128, r, 3), combo=i)
    # ... the other 3x3 geometries of that kernel
    for r in (64, 96, 128):
        for i, (pad, stride) in enumerate([(0, 1), (1, 2), (0, 2)]):
            for tag, n, per in ((f"m = {r} + 1", 1, r + 1), ("tiles straddle 3 images", 3, 35)):
                add(f"k32 3x3 rows {r}", f"pad {pad} stride {stride}, {tag}", geo_rows(C.K3, n, per, 64, 128, pad, stride), (r, 32, 0, 0),
                    (C.K32, 128, r, 3), combo=i)
    # k32 at BN = 64 (always 128 rows), one and three column blocks
    for name, kind, cin, ks in K32_KINDS:
        for i, (tag, n, per) in enumerate([("m = 127", 1, 127), ("m = 128", 1, 128), ("m = 129", 1, 129), ("tiles straddle 3 images", 3, 35),
                                           ("9 tiles", 1, 1025)]):
            add(f"k32 {name} BN 64", tag, geo_rows(kind, n, per, cin, 64 if i != 3 else 192, ks=ks), (-1, 32, 0, 0), (C.K32, 64, 128, 3), combo=i)
    # channels: one chunk (the shortest legal K loop), 128, 192 (chunk count no power of two); one and two 128-wide column blocks
    for name, kind, cmin, ks in K32_KINDS:
        for i, cin in enumerate(sorted({cmin, 128, 192})):
            for cout in (128, 256):
                add(f"k32 {name} channels", f"{cin} -> {cout}", geo_rows(kind, 2, 63, cin, cout, ks=ks), (64, 32, 0, 0), (C.K32, 128, 64, 3), combo=i)
    # 64-deep ring, KS = 3: NS 2 / 3 / 4
    for ns in (2, 3, 4):
        for i, (tag, n, per) in enumerate(row_edges(128)):
            add(f"ring NS {ns} 3x3", tag, geo_rows(C.K3, n, per, 64, 128), (-1, ns, 0, 0), (C.K64, 128, 128, ns), combo=i)
        for i, (cin, cout) in enumerate([(128, 64), (192, 192), (128, 256), (192, 128)]):
            add(f"ring NS {ns} 3x3", f"{cin} -> {cout}", geo_rows(C.K3, 2, 63, cin, cout), (-1, ns, 0, 0), (C.K64, C.conv_bn(cout), 128, ns), combo=i)
        for i, (pad, stride) in enumerate([(0, 1), (1, 2), (0, 2)]):
            add(f"ring NS {ns} 3x3", f"pad {pad} stride {stride}", geo_rows(C.K3, 3, 35, 64, 128, pad, stride), (-1, ns, 0, 0),
                (C.K64, 128, 128, ns), combo=i)
    # 64-deep, KS = 1: the default route at cin = 64, forced above; KS = 2: the only route of the 2x2 stride-2 conv
    for i, (tag, n, per) in enumerate(row_edges(128)):
        cout = (64, 128, 256, 192)[i % 4]
        add("ring 1x1", tag, geo_rows(C.K1, n, per, 64, cout), (-1, -1, -1, 0), (C.K64, C.conv_bn(cout), 128, 2), combo=i)
        add("ring 2x2s2", tag, geo_rows(C.K2S2, n, per, 64, cout), (-1, -1, -1, -1), (C.K64, C.conv_bn(cout), 128, 2), combo=i + 1)
    for i, cin in enumerate((128, 192)):
        add("ring 1x1", f"forced, {cin} -> 128", geo_rows(C.K1, 2, 63, cin, 128), (-1, -1, -1, 1), (C.K64, 128, 128, 2), combo=i)
        add("ring 2x2s2", f"{cin} -> 128", geo_rows(C.K2S2, 2, 63, cin, 128), (-1, -1, -1, -1), (C.K64, 128, 128, 2), combo=i)
    add("ring 2x2s2", "even extents", C.geo(C.K2S2, 2, 10, 6, 64, 64), (-1, -1, -1, -1), (C.K64, 64, 128, 2))
    # shared-A (3x3, pad 1, stride 1): BN 64 is the default rule at cin >= 128, BN 128 only forced
    for bn, cin, sa in ((64, 128, -1), (128, 64, 1)):
        for i, (tag, n, per) in enumerate(row_edges(128)):
            add(f"shared-A BN {bn}", tag, geo_rows(C.K3, n, per, cin, bn), (-1, -1, sa, 0), (C.SHARED_A, bn, 128, 2), combo=i)
        for i, (tag, h, w) in enumerate([("W = 1", 9, 1), ("W = 2", 70, 2), ("H = 1", 1, 131), ("H = W = 1", 1, 1)]):
            add(f"shared-A BN {bn}", tag, C.geo(C.K3, 2, h, w, cin, bn, 1, 1), (-1, -1, sa, 0), (C.SHARED_A, bn, 128, 2), combo=i)
    add("shared-A BN 64", "192 -> 192", geo_rows(C.K3, 2, 63, 192, 192), (-1, -1, -1, 0), (C.SHARED_A, 64, 128, 2))
    add("shared-A BN 64", "forced at 64 -> 64", geo_rows(C.K3, 3, 35, 64, 64), (-1, -1, 1, 0), (C.SHARED_A, 64, 128, 2), combo=1)
    add("shared-A BN 128", "192 -> 256", geo_rows(C.K3, 2, 63, 192, 256), (-1, -1, 1, 0), (C.SHARED_A, 128, 128, 2))
    # geometry, on the 32-deep kernel and the ring
    for fam, frc, exp in (("k32", (64, 32, 0, 0), (C.K32, 128, 64, 3)), ("ring NS 2", (-1, 2, 0, 0), (C.K64, 128, 128, 2))):
        geos = [("W = 1, pad 1", C.geo(C.K3, 2, 9, 1, 64, 128, 1, 1)), ("W = 2, pad 1", C.geo(C.K3, 2, 35, 2, 64, 128, 1, 1)),
                ("H = 1, pad 1", C.geo(C.K3, 2, 1, 67, 64, 128, 1, 1)), ("H = W = 3, pad 0: one output pixel", C.geo(C.K3, 1, 3, 3, 64, 128, 0, 1)),
                ("stride 2, odd x even, pad 1", C.geo(C.K3, 2, 11, 8, 64, 128, 1, 2)), ("stride 2, even x odd, pad 1", C.geo(C.K3, 2, 8, 11, 64, 128, 1, 2)),
                ("stride 2, odd x even, pad 0", C.geo(C.K3, 2, 11, 8, 64, 128, 0, 2)), ("stride 2, even x odd, pad 0", C.geo(C.K3, 2, 8, 11, 64, 128, 0, 2)),
                ("stride 2, W = 1, pad 1", C.geo(C.K3, 3, 6, 1, 64, 128, 1, 2))]
        for i, (tag, g) in enumerate(geos):
            add(f"{fam} 3x3 geometry", tag, g, frc, exp, combo=i)
    for ks, kc in ((3, 128), (4, 64)):
        for i, (tag, n, h, w) in enumerate([("1 x 1 source", 1, 1, 1), ("1 x 1 source, 3 images", 3, 1, 1), ("1 x W source", 2, 1, 9), ("H x 1 source", 2, 7, 1),
                                            ("odd source grid", 2, 3, 5), ("odd source grid, 2 tiles per class", 3, 5, 7)]):
            add(f"k32 up ks {ks} geometry", tag, C.geo(C.UP, n, h, w, kc, 128, ks=ks), (64, 32, 0, 0), (C.K32, 128, 64, 3), combo=i % 2)
    add("k32 4x4s2 geometry", "h = w = 2", C.geo(C.K4S2, 3, 2, 2, 64, 128), (64, 32, 0, 0), (C.K32, 128, 64, 3))
    add("k32 4x4s2 geometry", "2 x 18", C.geo(C.K4S2, 2, 2, 18, 128, 128), (96, 32, 0, 0), (C.K32, 128, 96, 3))
    # the rounding set: {-3..3} operands, sums past 256
    g128, g256 = geo_rows(C.K3, 3, 35, 128, 128), geo_rows(C.K3, 2, 63, 256, 256)
    for r in (64, 96, 128):
        add("rounding set", f"k32 rows {r}", g128, (r, 32, 0, 0), (C.K32, 128, r, 3), "rounded")
        add("rounding set", f"k32 rows {r}", g256, (r, 32, 0, 0), (C.K32, 128, r, 3), "rounded", combo=1)
    for ns in (2, 3, 4):
        add("rounding set", f"ring NS {ns}", g128, (-1, ns, 0, 0), (C.K64, 128, 128, ns), "rounded")
    add("rounding set", "shared-A BN 128", g256, (-1, -1, 1, 0), (C.SHARED_A, 128, 128, 2), "rounded")
    add("rounding set", "shared-A BN 64", geo_rows(C.K3, 3, 35, 128, 64), (-1, -1, -1, 0), (C.SHARED_A, 64, 128, 2), "rounded")
    add("rounding set", "k32 BN 64", geo_rows(C.K3, 3, 35, 128, 64), (-1, 32, 0, 0), (C.K32, 64, 128, 3), "rounded")
    add("rounding set", "1x1 k32", geo_rows(C.K1, 3, 35, 256, 256), (96, 32, 0, 0), (C.K32, 128, 96, 3), "rounded")
    add("rounding set", "up ks 4", C.geo(C.UP, 3, 5, 7, 128, 128, ks=4), (96, 32, 0, 0), (C.K32, 128, 96, 3), "rounded")
    add("rounding set", "up ks 3", C.geo(C.UP, 3, 5, 7, 256, 128, ks=3), (64, 32, 0, 0), (C.K32, 128, 64, 3), "rounded")
    add("rounding set", "4x4s2", geo_rows(C.K4S2, 3, 35, 128, 128), (128, 32, 0, 0), (C.K32, 128, 128, 3), "rounded")
    add("rounding set", "2x2s2", geo_rows(C.K2S2, 3, 35, 256, 128), (-1, -1, -1, -1), (C.K64, 128, 128, 2), "rounded")
    # the batch-norm backward epilogue (32-deep kernel only)
    for kind, name, cin in ((C.K3_BNBWD, "3x3", 64), (C.K1_BNBWD, "1x1", 128)):
        for r in (64, 96, 128):
            for act in (0, 1, 2):
                add(f"bnbwd {name}", f"act {act}, rows {r}, tiles straddle 3 images", geo_rows(kind, 3, 35, cin, 128), (r, 32, 0, 0), (C.K32, 128, r, 3), act=act)
            add(f"bnbwd {name}", f"act 1, m = {r} + 1, two column blocks", geo_rows(kind, 1, r + 1, cin, 256), (r, 32, 0, 0), (C.K32, 128, r, 3), act=1)
        for act in (1, 2):
            add(f"bnbwd {name}", f"act {act}, BN 64", geo_rows(kind, 1, 129, cin, 64), (-1, 32, 0, 0), (C.K32, 64, 128, 3), act=act)
    add("bnbwd 3x3", "act 2, pad 0", geo_rows(C.K3_BNBWD, 3, 35, 64, 128, 0, 1), (96, 32, 0, 0), (C.K32, 128, 96, 3), act=2)


_build()


@pytest.mark.parametrize("c", CASES, ids=[f"{i:03d}-{c.group.replace(' ', '_')}" for i, c in enumerate(CASES)])
def test_parity(c):
    run_case(c)


def test_case_tables_cover_every_instantiation():
    """every instantiation the launchers of conv2d_nhwc.hip can select is the asserted plan of at least one case (on the tables alone,
    whatever subset of the cases ran): conv3x3_k32<BN, MI, KS, UP>, conv3x3<BN, NS, KS>, conv3x3_p1<BN>, and the bnbwd epilogue"""
    have = {((c.g.kind, c.g.ks) + c.expect + (c.act is not None,)) for c in CASES}

    def need(kind, ks, family, bn, rows, ns, bb=False):
        assert (kind, ks, family, bn, rows, ns, bb) in have, (C.KIND_NAMES[kind], ks, C.FAMILY_NAMES[family], bn, rows, ns, bb)
    for kind, ks in ((C.K3, 3), (C.K1, 1), (C.UP, 3), (C.UP, 4), (C.K4S2, 4)):
        for rows in (64, 96, 128):
            need(kind, ks, C.K32, 128, rows, 3)
        need(kind, ks, C.K32, 64, 128, 3)
    for kind, ks in ((C.K3_BNBWD, 3), (C.K1_BNBWD, 1)):
        for rows in (64, 96, 128):
            need(kind, ks, C.K32, 128, rows, 3, True)
        need(kind, ks, C.K32, 64, 128, 3, True)
    for bn in (64, 128):
        for ns in (2, 3, 4):
            need(C.K3, 3, C.K64, bn, 128, ns)
        need(C.K1, 1, C.K64, bn, 128, 2)
        need(C.K2S2, 2, C.K64, bn, 128, 2)
        need(C.K3, 3, C.SHARED_A, bn, 128, 2)
    for kind in (C.K3, C.K1, C.UP, C.K2S2):   # with and without bias, with and without statistics
        assert {(c.bias, c.stats) for c in CASES if c.g.kind == kind and c.act is None} == set(COMBOS), C.KIND_NAMES[kind]
    assert len(CASES) < 450


# ---- weight images ----------------------------------------------------------------------------------------------------------------------
def _image(n):
    return torch.full((n,), float("nan"), dtype=C.BF, device=DEV)


@pytest.mark.parametrize("cin,cout", [(64, 128), (192, 64)])
def test_weight_images_agree_across_the_pack_entries(cin, cout):
    """3x3 and 1x1 layer: single pack (plain / transpose_flip, both weight memory orders), pair pack and the batch pack (a table mixing
    pairs, single images, 9-tap and 1-tap layers) give bit-equal images; the data-gradient image, used in a conv, gives the float64
    gradient exactly"""
    gen = torch.Generator().manual_seed(cin + cout)
    w3 = torch.randint(-1, 2, (cout, cin, 3, 3), generator=gen).float().to(DEV)
    w1 = torch.randint(-1, 2, (cout, cin, 1, 1), generator=gen).float().to(DEV)
    w3_nhwc = w3.permute(0, 2, 3, 1).contiguous()      # memory order [o][t][c]
    s = stream()
    img = {}
    for name, src, nhwc in (("nchw", w3, 0), ("nhwc", w3_nhwc, 1)):
        f, d = _image(w3.numel()), _image(w3.numel())
        assert L().s2d_conv2d3x3_pack_weights_bf16(p(src), cin, cout, 0, nhwc, p(f), s) == 0, last_error()
        assert L().s2d_conv2d3x3_pack_weights_bf16(p(src), cout, cin, 1, nhwc, p(d), s) == 0, last_error()
        pf, pd = _image(w3.numel()), _image(w3.numel())
        assert L().s2d_conv2d3x3_pack_weights_pair_bf16(p(src), cin, cout, nhwc, p(pf), p(pd), s) == 0, last_error()
        img[name] = (f, d, pf, pd)
    f1, d1, pf1, pd1 = (_image(w1.numel()) for _ in range(4))
    assert L().s2d_conv2d1x1_pack_weights_bf16(p(w1), cin, cout, 0, p(f1), s) == 0, last_error()
    assert L().s2d_conv2d1x1_pack_weights_bf16(p(w1), cout, cin, 1, p(d1), s) == 0, last_error()
    assert L().s2d_conv2d1x1_pack_weights_pair_bf16(p(w1), cin, cout, p(pf1), p(pd1), s) == 0, last_error()
    # the batch entry: pair 3x3 (nchw), single 1x1 forward, single 3x3 dgrad (nhwc), pair 1x1, single 3x3 forward (nhwc), single 1x1 dgrad
    b = [_image(w3.numel()) for _ in range(4)] + [_image(w1.numel()) for _ in range(4)]
    table = [(w3, cin, cout, 9, 0, 0, b[0], b[1]), (w1, cin, cout, 1, 0, 0, b[4], None), (w3_nhwc, cout, cin, 9, 1, 1, b[2], None),
             (w1, cin, cout, 1, 0, 0, b[5], b[6]), (w3_nhwc, cin, cout, 9, 1, 0, b[3], None), (w1, cout, cin, 1, 0, 1, b[7], None)]
    n = len(table)
    vp, i32 = ctypes.c_void_p * n, ctypes.c_int32 * n
    assert L().s2d_conv2d_pack_batch_bf16(n, vp(*[t[0].data_ptr() for t in table]), i32(*[t[1] for t in table]), i32(*[t[2] for t in table]),
                                          i32(*[t[3] for t in table]), i32(*[t[4] for t in table]), i32(*[t[5] for t in table]),
                                          vp(*[t[6].data_ptr() for t in table]), vp(*[None if t[7] is None else t[7].data_ptr() for t in table]),
                                          s) == 0, last_error()
    torch.cuda.synchronize()
    f, d = img["nchw"][0], img["nchw"][1]
    assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(d).all()) and not torch.equal(f, d)
    for name, t in (("pair fwd", img["nchw"][2]), ("nhwc single fwd", img["nhwc"][0]), ("nhwc pair fwd", img["nhwc"][2]), ("batch pair fwd", b[0]),
                    ("batch single fwd (nhwc)", b[3])):
        R.check_bits(t, f, "3x3 forward image, " + name, "element")
    for name, t in (("pair dgrad", img["nchw"][3]), ("nhwc single dgrad", img["nhwc"][1]), ("nhwc pair dgrad", img["nhwc"][3]), ("batch pair dgrad", b[1]),
                    ("batch single dgrad (nhwc)", b[2])):
        R.check_bits(t, d, "3x3 data-gradient image, " + name, "element")
    assert bool(torch.isfinite(f1).all()) and bool(torch.isfinite(d1).all())
    for name, t in (("pair", pf1), ("batch single", b[4]), ("batch pair", b[5])):
        R.check_bits(t, f1, "1x1 forward image, " + name, "element")
    for name, t in (("pair", pd1), ("batch pair", b[6]), ("batch single", b[7])):
        R.check_bits(t, d1, "1x1 data-gradient image, " + name, "element")
    # the data-gradient images in a conv: dx of y = conv(x, w) for an integer dy, against the float64 gradient
    for wt, dimg, kind, pad in ((w3, d, C.K3, 1), (w1, d1, C.K1, 0)):
        g = C.geo(kind, 2, 7, 9, cout, cin, pad, 1)
        dy = torch.randint(-1, 2, (g.n, cout, g.h, g.w), generator=gen).double()
        xr = torch.zeros(g.n, cin, g.h, g.w, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(xr, wt.double().cpu(), None, padding=pad).backward(dy)
        ref = C.nhwc_rows(xr.grad).round().long()
        force(64, 32, 0, 0)
        rc, plan = plan_of(g)
        assert rc == 0, last_error()
        xbuf, xd = C.fenced(C.nhwc_rows(dy), C.fence_rows(g), C.BF, DEV)
        ybuf, y = R.poisoned(C.out_pixels(g), g.cout, dtype=C.BF, device=DEV)
        assert launch(g, xd, dimg, None, y, None) == 0, last_error()
        torch.cuda.synchronize()
        C.check_case(g, plan, "exact", ref, ybuf.cpu(), what=f"{C.KIND_NAMES[kind]} data gradient through the transposed image")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _refused(g, frc, code, bb=False, what=""):
    """the entry answers `code` and writes nothing"""
    force(*frc)
    m = max(C.out_pixels(g), 1)
    x = torch.zeros(max(g.n * g.h * g.w, 1) * max(g.cin, 64), dtype=C.BF, device=DEV)
    packed = torch.zeros(max(g.ks * g.ks * g.cin * g.cout, 64), dtype=C.BF, device=DEV)
    ybuf, y = R.poisoned(m, max(g.cout, 64), dtype=C.BF, device=DEV)
    slabbuf, slabs = R.poisoned(m, 2, max(g.cout, 64), dtype=F32, device=DEV)
    z = torch.zeros(m * max(g.cout, 64), dtype=C.BF, device=DEV)
    sc = torch.ones(max(g.cout, 64), dtype=F32, device=DEV)
    rc = launch(g, x, packed, None, y, None if g.kind == C.K4S2 else slabs, (z, sc, sc, 1) if bb else None)
    torch.cuda.synchronize()
    assert rc == code, (what, rc, last_error())
    assert last_error()
    R.assert_untouched(ybuf, what + " y")
    R.assert_untouched(slabbuf, what + " slabs")


def test_refusals_write_nothing():
    _refused(C.geo(C.K3, 1, 5, 5, 96, 128, 1, 1), (-1,) * 4, R.S2D_ERR_UNSUPPORTED, what="3x3 cin 96")
    _refused(C.geo(C.K3, 1, 5, 5, 128, 100, 1, 1), (-1,) * 4, R.S2D_ERR_UNSUPPORTED, what="3x3 cout 100")
    _refused(C.geo(C.K1, 1, 5, 5, 32, 128), (-1,) * 4, R.S2D_ERR_UNSUPPORTED, what="1x1 cin 32")
    _refused(C.geo(C.K2S2, 1, 6, 6, 64, 96), (-1,) * 4, R.S2D_ERR_UNSUPPORTED, what="2x2s2 cout 96")
    _refused(C.geo(C.K4S2, 1, 6, 6, 64, 32), (-1,) * 4, R.S2D_ERR_UNSUPPORTED, what="4x4s2 cout 32")
    _refused(C.geo(C.K4S2, 1, 5, 6, 64, 128), (-1,) * 4, R.S2D_ERR_INVALID_ARG, what="4x4s2 odd h")
    _refused(C.geo(C.UP, 1, 3, 3, 64, 128, ks=3), (-1,) * 4, R.S2D_ERR_UNSUPPORTED, what="up ks 3 with kc = 64")
    _refused(C.geo(C.UP, 1, 3, 3, 128, 128, ks=5), (-1,) * 4, R.S2D_ERR_UNSUPPORTED, what="up ks 5")
    _refused(C.geo(C.K3_BNBWD, 1, 5, 5, 128, 64, 1, 1), (-1, 32, -1, 0), R.S2D_ERR_UNSUPPORTED, bb=True, what="3x3 bnbwd on the shared-A route")
    _refused(C.geo(C.K3_BNBWD, 1, 5, 5, 64, 128, 1, 1), (-1, 2, 0, 0), R.S2D_ERR_UNSUPPORTED, bb=True, what="3x3 bnbwd on the 64-deep ring")
    _refused(C.geo(C.K1_BNBWD, 1, 5, 5, 64, 128), (-1,) * 4, R.S2D_ERR_UNSUPPORTED, bb=True, what="1x1 bnbwd at cin 64 (64-deep route)")
    _refused(C.geo(C.K1_BNBWD, 1, 5, 5, 128, 128), (-1, -1, -1, 1), R.S2D_ERR_UNSUPPORTED, bb=True, what="1x1 bnbwd with the 64-deep route forced")
    # ... and the queries say so beforehand, from the same plan
    force(-1, 2, 0, 0)
    assert raw("s2d_conv2d3x3_bnbwd_supported")(64, 128, 1, 1) == 0
    force(-1, 32, 0, 0)
    assert raw("s2d_conv2d3x3_bnbwd_supported")(64, 128, 1, 1) == 1 and raw("s2d_conv2d3x3_bnbwd_supported")(64, 128, 1, 2) == 0
    force(-1, 32, -1, 0)
    assert raw("s2d_conv2d3x3_bnbwd_supported")(128, 64, 1, 1) == 0 and raw("s2d_conv2d3x3_bnbwd_supported")(128, 64, 0, 1) == 1
    assert raw("s2d_conv2d1x1_bnbwd_supported")(64, 128) == 0 and raw("s2d_conv2d1x1_bnbwd_supported")(128, 64) == 1
    assert L().s2d_conv2d_debug_force(100, -1, -1, -1) == R.S2D_ERR_INVALID_ARG


def test_zz_report(capsys):
    """prints the plan table of the forced sweeps, the largest |ref| per case group and the GELU error / bound ratio (the source of
    profiles/conv2d_parity.txt); asserts nothing beyond the exact-set condition that every case already asserted"""
    with capsys.disabled():
        print()
        for (group, _), line in sorted(LINES.items(), key=lambda kv: kv[0][0]):
            print("PLAN  " + line)
        for group, top in sorted(TOPS.items()):
            print(f"MAXREF  {group:<28} {top}")
        for fam, worst in sorted(R.WORST.items()):
            print(f"RATIO  {fam}: worst |err| / bound = {worst:.4f}")
    assert all(top <= C.EXACT_MAX for group, top in TOPS.items() if group != "rounding set")
