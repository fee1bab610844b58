"""Exact parity of every dense 2-D weight-gradient kernel of csrc/conv2d_wgrad.hip at every ring depth, K-loop length and split plan,
called through _lib.load() with raw pointers.  References, the plan mirror, the checkers and the reasoning behind them:
tests/conv2d_wgrad_ref.py; tests/test_conv2d_wgrad_checks_cpu.py shows that the checkers can fail.

Every case forces its plan with s2d_conv2d_wgrad_debug_force (include/s2d_debug.h), asserts that the plan report s2d_conv2d_wgrad_plan
equals the mirror and shows the TCO, TCI, NS, splits and K-steps per workgroup the case is for, that the entry's own workspace query
(asked unmemoised through fn.__wrapped__) is the size of that many slabs, then launches twice from operands between NaN fences into
fresh NaN-filled, guarded dweight / dbias / workspace: the two results are bit-equal, every element is written, every guard intact, and
dW, every per-split slab, every per-split bias row and dbias are torch.equal to the integer reference.  No comparison is bounded.  The
override is restored after every test.

test_case_tables_cover_every_instantiation asserts, on the tables alone, that all 32 instantiations (4 entries x 4 channel-tile pairs x
2 ring depths) have a case and that, for every ring depth NS the mirror reports, workgroups of 1, 2, NS - 2, NS - 1, NS, NS + 1 and
2 NS + 1 K-steps and a short last split are launched.

Stride 2: the tap column 2 j - 1 + kx reaches -1 for both kernel sizes and W only for ks = 4 (ks = 3 ends at W - 1 on an even W).
"""
import collections
import ctypes
import functools
import os

import pytest
import torch

import bn_pass_ref as R
import conv2d_wgrad_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
LINES = {}      # (case group, entry, TCO, TCI, NS) -> the plan line of its first case (test_zz_report prints them: profiles/conv2d_wgrad_parity.txt)
TOPS = {}       # case group -> largest |ref|


def _env_deep():
    """S2D_WG_RING_DEEP as the library reads it (atoi; unset = the deep ring)"""
    e = os.environ.get("S2D_WG_RING_DEEP")
    if e is None:
        return True
    try:
        return int(e) != 0
    except ValueError:
        return False


ENV_DEEP = _env_deep()


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


def force(deep=-1, splits=-1):
    assert L().s2d_conv2d_wgrad_debug_force(deep, splits) == 0, last_error()


@pytest.fixture(autouse=True)
def _restore_plan():
    try:
        yield
    finally:
        force()


def plan_of(g):
    out = (ctypes.c_int32 * 8)()
    rc = L().s2d_conv2d_wgrad_plan(g.kind, g.n, g.h, g.w, g.cin, g.cout, g.pad, g.ks, out)
    return rc, W.Plan(*list(out))


@functools.lru_cache(maxsize=None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def zero_page():
    return torch.zeros(64, dtype=torch.uint8, device=DEV)


def ws_query(g):
    """the entry's own workspace query (unmemoised), in bytes"""
    if g.kind == W.K3:
        return raw("s2d_conv2d3x3_wgrad_workspace_bytes")(g.n, g.h, g.w, g.cin, g.cout, g.pad)
    if g.kind == W.K1:
        return raw("s2d_conv2d1x1_wgrad_workspace_bytes")(g.n, g.h, g.w, g.cin, g.cout)
    return raw("s2d_conv2d_s2_wgrad_workspace_bytes")(g.n, g.h, g.w, g.cout, g.cin, g.ks)


def launch(g, x, dy, dw, db, ws, ws_bytes):
    """one call of the entry of g with raw pointers -> its return code (stride 2: a = dy's tensor, ca = cout; b = x, cb = cin)"""
    zp, s = p(zero_page()), stream()
    if g.kind == W.K3:
        return L().s2d_conv2d3x3_wgrad_nhwc_bf16(p(x), p(dy), zp, g.n, g.h, g.w, g.cin, g.cout, g.pad, p(dw), p(db), p(ws), ws_bytes, s)
    if g.kind == W.K1:
        return L().s2d_conv2d1x1_wgrad_nhwc_bf16(p(x), p(dy), zp, g.n, g.h, g.w, g.cin, g.cout, p(dw), p(db), p(ws), ws_bytes, s)
    assert db is None
    return L().s2d_conv2d_s2_wgrad_nhwc_bf16(p(dy), p(x), zp, g.n, g.h, g.w, g.cout, g.cin, g.ks, p(dw), p(ws), ws_bytes, s)


@functools.lru_cache(maxsize=None)
def operands(g, seed):
    """float64 integer operands, built once per (geometry, seed) and never modified"""
    return W.int_operands(g, seed)


Case = collections.namedtuple("Case", "group tag g deep splits db seed")


def run_case(c, expect_steady=False):
    g = c.g
    force(-1 if c.deep is None else int(c.deep), -1 if c.splits is None else c.splits)
    deep = ENV_DEEP if c.deep is None else c.deep
    rc, plan = plan_of(g)
    assert rc == 0, last_error()
    want = W.mirror_plan(g, cus(), deep, c.splits)
    assert plan == want, f"{c.tag}: the plan report {plan} is not the mirror's {want}"
    if c.splits is not None:   # the plan this case is for, as its table entry was built (independent of the CU count)
        assert plan == W.mirror_plan(g, 256, deep, c.splits)
    assert (plan.tco, plan.tci) == (W.tile_of(g.cout), W.tile_of(g.cin)) and plan.ns == W.cfg(plan.tco, plan.tci, g.ks, W.stride_of(g), deep).ns
    assert plan.splits * plan.spb >= W.total_steps(g) > (plan.splits - 1) * plan.spb
    if expect_steady:
        assert plan.spb > plan.ns, f"{c.tag}: the default plan {plan} never leaves the prologue"
    ws_bytes = ws_query(g)
    assert ws_bytes == 4 * W.ws_floats(g, plan), (c.tag, ws_bytes, plan)
    x, dy = operands(g, c.seed)
    fx, fd = W.fences(g)
    xbuf, xd = W.fenced(W.nhwc_flat(x), fx, W.BF, DEV)
    dybuf, dyd = W.fenced(W.nhwc_flat(dy), fd, W.BF, DEV)
    outs = []
    for _ in range(2):
        (dwbuf, dw), (dbbuf, db), (wsbuf, ws) = W.out_buffers(g, plan, c.db, DEV)
        rc = launch(g, xd, dyd, dw, db, ws, ws_bytes)
        assert rc == 0, (c.tag, last_error())
        torch.cuda.synchronize()
        outs.append((dwbuf, dbbuf, wsbuf))
    R.check_bits(outs[0][0], outs[1][0], c.tag + ": dweight of the two launches", "co, ci x tap")
    R.check_bits(outs[0][2], outs[1][2], c.tag + ": workspace of the two launches", "row, column")
    if c.db:
        R.check_bits(outs[0][1], outs[1][1], c.tag + ": dbias of the two launches", "row, column")
    dwbuf, dbbuf, wsbuf = outs[0]
    top = W.check_case(g, plan, x, dy, dwbuf.cpu(), None if dbbuf is None else dbbuf.cpu(), wsbuf.cpu(), what=c.tag)
    TOPS[c.group] = max(TOPS.get(c.group, 0), top)
    LINES.setdefault((c.group, W.entry_of(g), plan.tco, plan.tci, plan.ns), W.plan_line(c.tag, g, plan, deep))
    return plan


# ---- case tables ------------------------------------------------------------------------------------------------------------------------
ENTRIES = [(W.K3, 3), (W.K1, 1), (W.S2, 3), (W.S2, 4)]     # the four entries as they dispatch
CASES = []


def rows_geo(kind, ks, n, ho, wo, cin, cout, pad=1):
    """the entry arguments whose output (the grid the K-steps walk) is n x ho x wo"""
    if kind == W.K1:
        return W.geo(kind, n, ho, wo, cin, cout)
    if kind == W.K3:
        return W.geo(kind, n, ho + 2 - 2 * pad, wo + 2 - 2 * pad, cin, cout, pad)
    return W.geo(kind, n, 2 * ho, 2 * wo, cin, cout, ks=ks)


def add(group, tag, g, deep, splits, db=True, seed=0):
    assert W.supported(g), g
    db = db and g.kind != W.S2
    CASES.append(Case(group, f"{group}: {tag} [{W.ENTRY_NAMES[W.entry_of(g)]} {g.n}x{g.h}x{g.w} {g.cin}->{g.cout} p{g.pad}]", g, deep, splits, db, seed))


def block_lengths(c):
    """K-steps of each workgroup column of a forced case (from the mirror)"""
    plan = W.mirror_plan(c.g, 256, c.deep, c.splits)
    return plan, [s1 - s0 for s0, s1 in W.split_ranges(c.g, plan)]


def ns_carriers():
    """for every ring depth the mirror reports: an (entry, cin, cout, deep) that has it, preferring single tiles"""
    out = {}
    for deep in (False, True):
        for kind, ks in ENTRIES:
            for cout in (64, 128):
                for cin in (64, 128):
                    ns = W.cfg(cout, cin, ks, 2 if kind == W.S2 else 1, deep).ns
                    out.setdefault(ns, (kind, ks, cin, cout, deep))
    return out


def n_edges(ns):
    return sorted({1, 2, ns - 2, ns - 1, ns, ns + 1, 2 * ns + 1})


def _build():
    # A. all 32 instantiations; channels {64, 128, 192, 256}: a tile size on one axis with one tile, two or three on the other (3 x 1,
    #    1 x 3, 2 x 1, 1 x 2 tiles: the cot / cit decode of blockIdx.z is no bijection if it divides by the wrong count); 12 K-steps
    many = {64: 192, 128: 256}
    for kind, ks in ENTRIES:
        for tco in (64, 128):
            for tci in (64, 128):
                add("instantiations", f"TCO {tco} TCI {tci} deep", rows_geo(kind, ks, 2, 3, 40, tci, many[tco]), True, 1, seed=1)
                add("instantiations", f"TCO {tco} TCI {tci} four-slot", rows_geo(kind, ks, 2, 3, 40, many[tci], tco), False, 1, seed=2)
    add("instantiations", "3 x 3 tiles", rows_geo(W.K3, 3, 2, 3, 40, 192, 192), True, 2)
    add("instantiations", "2 x 2 tiles", rows_geo(W.S2, 4, 2, 3, 40, 256, 256), True, 2)
    add("instantiations", "1 x 2 tiles of 128 x 64", rows_geo(W.K1, 1, 2, 3, 40, 128, 256), False, 2)
    # B. K-steps per workgroup around every ring depth: two images of n output rows, one 32-pixel block per row, two splits -> each
    #    workgroup walks n steps and the second starts exactly on the image boundary; the short last split from a search of the mirror
    for ns, (kind, ks, cin, cout, deep) in sorted(ns_carriers().items()):
        for i, n in enumerate(n_edges(ns)):
            add(f"K loop NS {ns}", f"n = {n}", rows_geo(kind, ks, 2, n, 20 + i, cin, cout, pad=i % 2), deep, 2, db=i % 2 == 0, seed=i)
        found = None
        for ho in range(ns, 3 * ns):
            g = rows_geo(kind, ks, 2, ho, 20, cin, cout)
            plan = W.mirror_plan(g, 256, deep, 3)
            if plan.splits == 3 and plan.spb > ns and W.total_steps(g) % plan.spb not in (0,) and W.total_steps(g) - 2 * plan.spb < plan.spb:
                found = g
                break
        assert found is not None, ns
        add(f"K loop NS {ns}", "short last split", found, deep, 3)
    # C. fold sizes: each of the four thread rows of the reduce folds 0, 1 and several slabs
    for s in (1, 2, 3, 4, 5, 10):
        add("fold", f"{s} splits", W.geo(W.K3, 1, 5, 40, 64, 64, 1), True, s)
    add("fold", "20 splits", W.geo(W.K3, 2, 5, 40, 64, 64, 1), True, 20)
    add("fold", "9 splits", rows_geo(W.S2, 3, 1, 9, 20, 64, 64), True, 9)
    add("fold", "13 splits", W.geo(W.K1, 1, 13, 20, 64, 128), False, 13)
    # D. step walk: three images of 3 rows x 2 column blocks (18 steps); splits of 3, 4 and 5 steps begin mid-row, mid-image and on an
    #    image boundary
    for want, spb in ((6, 3), (5, 4), (4, 5)):
        add("step walk", f"{spb} steps per split", rows_geo(W.K3, 3, 3, 3, 40, 64, 64), True, want, seed=spb)
    for kind, ks in ENTRIES[1:]:
        add("step walk", "5 steps per split", rows_geo(kind, ks, 3, 3, 40, 64, 64), False, 4)
    # E. row geometry of the stride-1 entries
    for i, wo in enumerate((1, 31, 32, 33, 70)):
        for pad in (0, 1):
            add("row geometry", f"Wo = {wo}, pad {pad}", rows_geo(W.K3, 3, 2, 4, wo, 64, 64, pad), bool((i + pad) % 2), 2, db=pad == 1, seed=wo)
        add("row geometry", f"Wo = {wo}", rows_geo(W.K1, 1, 2, 2, wo, 64, 64), bool(i % 2), 2, seed=wo)
    add("row geometry", "H = 1, pad 1", W.geo(W.K3, 2, 1, 33, 64, 64, 1), True, 2)
    add("row geometry", "H = 1, pad 1, four-slot", W.geo(W.K3, 3, 1, 70, 128, 64, 1), False, 3)
    add("row geometry", "H = 3, pad 0: Ho = 1", W.geo(W.K3, 2, 3, 35, 64, 64, 0), True, 2)
    add("row geometry", "H = W = 3, pad 0: one output pixel", W.geo(W.K3, 1, 3, 3, 64, 128, 0), True, 1)
    # F. stride 2
    for ks in (3, 4):
        for i, (h, w) in enumerate(((2, 2), (4, 64), (4, 66), (6, 2), (2, 140))):
            cin, cout = ((64, 64), (128, 64), (64, 128), (128, 128), (192, 64))[i]
            add("stride 2", f"ks {ks}, {h} x {w}", W.geo(W.S2, 2, h, w, cin, cout, ks=ks), bool(i % 2), 2, seed=ks + i)
    # G. bias gradient: one, two and three input-channel tiles (only ci tile 0 of kernel row 0 contributes), several output-channel tiles
    for kind, ks in ENTRIES[:2]:
        for i, (cin, cout) in enumerate(((64, 192), (256, 256), (192, 256), (256, 64), (192, 192))):
            add("bias gradient", f"{cin} -> {cout}, dbias", rows_geo(kind, ks, 2, 3, 40, cin, cout), bool(i % 2), 3, db=True, seed=i)
        add("bias gradient", "192 -> 256, dbias NULL", rows_geo(kind, ks, 2, 3, 40, 192, 256), True, 3, db=False)
        add("bias gradient", "64 -> 64, dbias NULL", rows_geo(kind, ks, 2, 3, 40, 64, 64), False, 3, db=False)


_build()
FORCED = list(CASES)


@pytest.mark.parametrize("c", FORCED, ids=[f"{i:03d}-{c.group.replace(' ', '_')}" for i, c in enumerate(FORCED)])
def test_parity(c):
    run_case(c)


def test_case_tables_cover_every_instantiation():
    """on the tables alone, whatever subset of the cases ran"""
    have = {(W.entry_of(c.g), W.tile_of(c.g.cout), W.tile_of(c.g.cin), c.deep) for c in FORCED}
    need = {(e, tco, tci, deep) for e in range(4) for tco in (64, 128) for tci in (64, 128) for deep in (False, True)}
    assert len(need) == 32 and need <= have, sorted(need - have)
    # each tile size with two or three tiles on its axis, and unequal tile counts on the two axes
    assert {(W.tile_of(c.g.cout), c.g.cout // W.tile_of(c.g.cout)) for c in FORCED} >= {(64, 1), (64, 3), (128, 1), (128, 2)}
    assert {(W.tile_of(c.g.cin), c.g.cin // W.tile_of(c.g.cin)) for c in FORCED} >= {(64, 1), (64, 3), (128, 1), (128, 2)}
    # K-steps per workgroup around every ring depth the mirror reports
    depths = {W.cfg(tco, tci, ks, 2 if kind == W.S2 else 1, deep).ns for kind, ks in ENTRIES for tco in (64, 128) for tci in (64, 128) for deep in (False, True)}
    assert depths == set(ns_carriers()) and 4 in depths and len(depths) >= 2
    lengths, short = collections.defaultdict(set), set()
    for c in FORCED:
        plan, ns_ = block_lengths(c)
        lengths[plan.ns] |= set(ns_)
        if ns_[-1] < plan.spb and plan.spb > plan.ns:
            short.add(plan.ns)
    for ns in depths:
        assert set(n_edges(ns)) <= lengths[ns], (ns, sorted(set(n_edges(ns)) - lengths[ns]))
        assert ns in short, ns
    # fold sizes, split boundaries, row geometry, stride-2 widths, bias gradient
    folds = {block_lengths(c)[0].splits for c in FORCED}
    assert {1, 2, 3, 4, 5} <= folds and max(folds) >= 9
    kinds = set()
    for c in FORCED:
        if c.g.n >= 2:
            kinds |= W.boundary_kinds(c.g, block_lengths(c)[0])
    assert kinds == {"mid-row", "mid-image", "image"}
    for pad in (0, 1):
        assert {W.out_hw(c.g)[1] for c in FORCED if c.g.kind == W.K3 and c.g.pad == pad} >= {1, 31, 32, 33, 70}
    assert any(c.g.kind == W.K3 and c.g.h == 1 and c.g.pad == 1 for c in FORCED) and any(c.g.kind == W.K3 and c.g.h == 3 and c.g.pad == 0 for c in FORCED)
    for ks in (3, 4):
        assert {(c.g.h, c.g.w) for c in FORCED if c.g.kind == W.S2 and c.g.ks == ks} >= {(2, 2), (4, 64), (4, 66)}
    for kind in (W.K3, W.K1):
        tiles = {c.g.cin // W.tile_of(c.g.cin) for c in FORCED if c.g.kind == kind and c.db and c.g.cout // W.tile_of(c.g.cout) > 1}
        assert tiles >= {1, 2, 3}, (kind, tiles)
        assert {c.db for c in FORCED if c.g.kind == kind} == {True, False}
    assert len(FORCED) < 200


def test_outside_kernel_rows_are_exact_zero_slabs():
    """H = 1 with pad 1: kernel rows 0 and 2 lie entirely outside the image; their slabs of every split are written, and are zeros"""
    g = W.geo(W.K3, 2, 1, 33, 64, 64, 1)
    force(1, 2)
    rc, plan = plan_of(g)
    assert rc == 0 and plan.splits == 2
    x, dy = operands(g, 0)
    slabs, _ = W.slab_references(g, plan, x, dy)
    assert not bool(slabs[:, 0].any()) and not bool(slabs[:, 2].any()) and bool(slabs[:, 1].any())
    fx, fd = W.fences(g)
    _, xd = W.fenced(W.nhwc_flat(x), fx, W.BF, DEV)
    _, dyd = W.fenced(W.nhwc_flat(dy), fd, W.BF, DEV)
    (dwbuf, dw), _, (wsbuf, ws) = W.out_buffers(g, plan, False, DEV)
    assert launch(g, xd, dyd, dw, None, ws, ws_query(g)) == 0, last_error()
    torch.cuda.synchronize()
    got = ws.reshape(-1)[:slabs.numel()].reshape(slabs.shape).cpu()
    assert torch.equal(got[:, 0], torch.zeros_like(got[:, 0])) and torch.equal(got[:, 2], torch.zeros_like(got[:, 2]))


# ---- the shipped plan's steady state ------------------------------------------------------------------------------------------------
UNFORCED = [("3x3 s1", W.K3, 3, 64, 64, (4, 64, 96)), ("1x1", W.K1, 1, 256, 256, (4, 32, 160)), ("3x3 s2", W.S2, 3, 64, 64, (4, 64, 96)),
            ("4x4 s2", W.S2, 4, 64, 64, (4, 32, 96))]


@pytest.mark.parametrize("name,kind,ks,cin,cout,out", UNFORCED, ids=[u[0].replace(" ", "_") for u in UNFORCED])
def test_default_plan_steady_state(name, kind, ks, cin, cout, out):
    """nothing forced: the smallest of a few map heights at which the DEFAULT plan (from the report, whatever the CU count) gives a
    workgroup more K-steps than its ring has slots, so the shipped plan's steady state gets an exact check too"""
    force()
    n, ho, wo = out
    for mult in (1, 2, 4):
        g = rows_geo(kind, ks, n, ho * mult, wo, cin, cout)
        rc, plan = plan_of(g)
        assert rc == 0, last_error()
        if plan.spb > plan.ns:
            break
    else:
        pytest.skip(f"{cus()} CUs: no candidate map gives the default plan more than NS K-steps per workgroup (last plan {plan})")
    plan = run_case(Case("default plan", f"default plan: {name} [{g.n}x{g.h}x{g.w} {g.cin}->{g.cout}]", g, None, None, kind != W.S2, 5), expect_steady=True)
    assert plan.spb > plan.ns


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _refused(g, code, what, short_by=0, db=True):
    """the entry answers `code` and writes nothing"""
    ho, wo = max(W.out_hw(g)[0], 1), max(W.out_hw(g)[1], 1)
    x = torch.zeros(max(g.n, 1) * max(g.h, 1) * max(g.w, 1) * max(g.cin, 64), dtype=W.BF, device=DEV)
    dy = torch.zeros(max(g.n, 1) * ho * wo * max(g.cout, 64), dtype=W.BF, device=DEV)
    dwbuf, dw = R.poisoned(max(g.cout, 64), max(g.cin, 64) * g.ks * g.ks, dtype=F32, device=DEV)
    dbbuf, dbias = R.poisoned(4, 64, dtype=F32, device=DEV)
    ws_bytes = ws_query(g) if W.supported(g) else 1 << 20
    wsbuf, ws = R.poisoned(W.ceil_div(ws_bytes, 256), 64, dtype=F32, device=DEV)
    rc = launch(g, x, dy, dw, dbias if db and g.kind != W.S2 else None, ws, ws_bytes - short_by)
    torch.cuda.synchronize()
    assert rc == code, (what, rc, last_error())
    assert last_error()
    for buf, name in ((dwbuf, "dweight"), (dbbuf, "dbias"), (wsbuf, "workspace")):
        R.assert_untouched(buf, f"{what} {name}")
    out = (ctypes.c_int32 * 8)()
    if short_by == 0:   # ... and the plan report refuses the same arguments
        assert L().s2d_conv2d_wgrad_plan(g.kind, g.n, g.h, g.w, g.cin, g.cout, g.pad, g.ks, out) == R.S2D_ERR_UNSUPPORTED, what
        assert ws_query(g) == 0, what


def test_refusals_write_nothing():
    force()
    _refused(W.geo(W.K3, 1, 5, 5, 96, 128, 1), R.S2D_ERR_UNSUPPORTED, "3x3 cin 96")
    _refused(W.geo(W.K3, 1, 5, 5, 128, 32, 1), R.S2D_ERR_UNSUPPORTED, "3x3 cout 32")
    _refused(W.geo(W.K1, 1, 5, 5, 100, 128), R.S2D_ERR_UNSUPPORTED, "1x1 cin 100")
    _refused(W.geo(W.S2, 1, 6, 6, 64, 96, ks=3), R.S2D_ERR_UNSUPPORTED, "s2 ca 96")
    _refused(W.geo(W.S2, 1, 6, 6, 64, 64, ks=2), R.S2D_ERR_UNSUPPORTED, "s2 ks 2")
    _refused(W.geo(W.S2, 1, 5, 6, 64, 64, ks=3), R.S2D_ERR_INVALID_ARG, "s2 odd h")
    _refused(W.geo(W.S2, 1, 6, 7, 64, 64, ks=4), R.S2D_ERR_INVALID_ARG, "s2 odd w")
    _refused(W.geo(W.K3, 1, 2, 9, 64, 64, 0), R.S2D_ERR_INVALID_ARG, "3x3 pad 0 on two rows: empty output")
    _refused(W.geo(W.K3, 1, 9, 1, 64, 64, 0), R.S2D_ERR_INVALID_ARG, "3x3 pad 0 on one column: empty output")
    for g in (W.geo(W.K3, 2, 5, 40, 64, 64, 1), W.geo(W.K1, 2, 5, 40, 64, 64), W.geo(W.S2, 2, 6, 40, 64, 64, ks=4)):
        _refused(g, R.S2D_ERR_WORKSPACE, f"{W.ENTRY_NAMES[W.entry_of(g)]} workspace one byte short", short_by=1)
    # bad force values change nothing
    force(0, 3)
    g = W.geo(W.K3, 1, 5, 40, 64, 64, 1)
    before = plan_of(g)
    for bad in ((2, -1), (-2, -1), (-1, 0), (-1, -2), (1, 1 << 20)):
        assert L().s2d_conv2d_wgrad_debug_force(*bad) == R.S2D_ERR_INVALID_ARG, bad
        assert plan_of(g) == before and before[1].ns == 4 and before[1].splits == 3
    # the override reaches the workspace queries too
    assert ws_query(g) == 4 * W.ws_floats(g, before[1])
    force()
    assert ws_query(g) == 4 * W.ws_floats(g, W.mirror_plan(g, cus(), ENV_DEEP))


def test_zz_report(capsys):
    """prints one plan line per distinct plan of every case group and the largest |ref| per group (the source of
    profiles/conv2d_wgrad_parity.txt); asserts nothing beyond the exact-set condition that every case already asserted"""
    with capsys.disabled():
        print()
        for _, line in sorted(LINES.items(), key=lambda kv: kv[0]):
            print("PLAN  " + line)
        for group, top in sorted(TOPS.items()):
            print(f"MAXREF  {group:<20} {top}")
        print(f"CASES  {len(FORCED)} forced + {len(UNFORCED)} default-plan; comparisons: torch.equal only")
    assert all(top < 2 ** 24 for top in TOPS.values())
