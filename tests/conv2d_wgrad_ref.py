"""TEST INFRASTRUCTURE ONLY - exact references, a launch-plan mirror, checkers and a host emulation for the dense 2-D weight-gradient
kernels of csrc/conv2d_wgrad.hip (s2d_conv2d3x3_wgrad / s2d_conv2d1x1_wgrad / s2d_conv2d_s2_wgrad with ks 3 and 4, and the bias gradient
that rides on the first two).  Imports without a GPU and never loads the native library: tests/test_conv2d_wgrad_parity_gpu.py drives
the entries, tests/test_conv2d_wgrad_checks_cpu.py shows on the host that every checker below can fail.

Method.  Nothing below is fitted to what the kernels return, and no comparison in this file is bounded: all are torch.equal.
  operands: both tensors hold seeded random integers in {-3..3} (exact in bf16), so every (co, ci, ky, kx) has its own expected value.
  reference: torch conv2d / conv_transpose2d autograd in float64 on the host (exact at these magnitudes), cast to int64.  It knows
      nothing of splits, tiles or K-steps.  The exactness condition, asserted ON THE REFERENCE ALONE (assert_exact_condition):
      9 * n * Ho * Wo < 2^24 and max|ref| < 2^24.  Every product is an integer of magnitude <= 9 and an output sums at most
      n * Ho * Wo of them, so every partial sum - of one MFMA accumulator, one split's slab, a row of the four-row fold, the dbias
      shuffles - is an integer below 2^24 in magnitude whatever the order, i.e. exact in fp32.
  per-split slabs: the workspace holds one [ky][kx][co][ci] slab per split and, when dbias is asked for, one [co] row per split behind
      them.  Their expected values are the same contraction restricted to the output pixels of the split's K-steps (membership from the
      plan report: step s = (image, output row, 32-pixel column block)); the slabs' sum is asserted to be the autograd reference.
      Without dbias the rows behind the slabs must keep their NaN fill.
  fencing: x and dY each sit in the middle of a NaN-filled allocation ((W + 3) * channels elements on each side of x, 33 * channels on
      each side of dY), so an out-of-image fetch the zero page does not replace is a NaN in dW.  dweight, dbias and the workspace
      (exactly the queried size) are NaN-filled with guard rows (poisoned / assert_written of bn_pass_ref.py): every element written,
      every guard intact.

Naming: `cin` / `cout` are the kernel's roles - cin = channels of the tensor the taps walk over (x; b of the stride-2 entry, [n][h][w]),
cout = channels of the other one (dY; a of the stride-2 entry, [n][Ho][Wo]); dW is [cout][cin][ks][ks].
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

import bn_pass_ref as R

K3, K1, S2 = 0, 1, 2
KIND_NAMES = ("3x3", "1x1", "s2")
BF = torch.bfloat16
LDS_BYTES = 160 * 1024
ENTRY_NAMES = ("3x3 s1", "1x1", "3x3 s2", "4x4 s2")

Geo = namedtuple("Geo", "kind n h w cin cout pad ks")
Plan = namedtuple("Plan", "tco tci ns kxn splits spb gy gz")
Cfg = namedtuple("Cfg", "cpr_a cpr_b a_chunks nb b_chunks chunks ns_fit ns nu nl")


def geo(kind, n, h, w, cin, cout, pad=None, ks=None):
    """the plan report's arguments; pad / ks filled in for the kinds that fix them"""
    if kind == K1:
        pad, ks = 0, 1
    elif kind == K3:
        ks = 3
    else:
        pad = 1
    return Geo(kind, n, h, w, cin, cout, pad, ks)


def ceil_div(a, b):
    return -(-a // b)


def stride_of(g):
    return 2 if g.kind == S2 else 1


def entry_of(g):
    """index into ENTRY_NAMES: the four entries as they dispatch"""
    return g.kind if g.kind != S2 else (3 if g.ks == 4 else 2)


def out_hw(g):
    s = stride_of(g)
    return (g.h + 2 * g.pad - g.ks) // s + 1, (g.w + 2 * g.pad - g.ks) // s + 1


def total_steps(g):
    ho, wo = out_hw(g)
    return g.n * ho * ceil_div(wo, 32)


# ---- WgCfg and wg_plan, restated ------------------------------------------------------------------------------------------------------
def cfg(tco, tci, ks, stride, deep):
    """WgCfg<TCO, TCI, KS, STRIDE, DEEP>: 16-byte chunks per staged pixel row (data + pad), chunk counts of the A (32 pixels) and B
    (31 * stride + ks pixels) tiles rounded to whole waves, the ring depth, and what the K loop derives from them: NU = chunk rounds of
    the 512 threads, nl[wave] = global_load_lds instructions the wave issues per K-step (the unit of its vmcnt waits)"""
    cpr_a, cpr_b = tco // 8 + 2, tci // 8 + (1 if stride == 2 else 2)
    a_chunks = ceil_div(32 * cpr_a, 64) * 64
    nb = 31 * stride + (3 if ks == 1 else ks)
    b_chunks = ceil_div(nb * cpr_b, 64) * 64
    chunks = a_chunks + b_chunks
    ns_fit = LDS_BYTES // (16 * chunks)
    ns = min(ns_fit, 8) if deep else 4
    nu = ceil_div(chunks, 512)
    nl = tuple(sum(1 for u in range(nu) if 64 * wave + 512 * u < chunks) for wave in range(8))
    assert ns >= 4 and all(1 <= v <= 4 for v in nl)
    return Cfg(cpr_a, cpr_b, a_chunks, nb, b_chunks, chunks, ns_fit, ns, nu, nl)


def tile_of(c):
    return 128 if c % 128 == 0 else 64


def supported(g):
    if g.cin % 64 or g.cout % 64 or g.cin < 64 or g.cout < 64 or g.n <= 0 or g.h <= 0 or g.w <= 0:
        return False
    if g.kind == K3:
        return g.ks == 3 and g.pad in (0, 1) and g.h + 2 * g.pad - 2 > 0 and g.w + 2 * g.pad - 2 > 0
    if g.kind == K1:
        return g.ks == 1 and g.pad == 0
    return g.ks in (3, 4) and g.pad == 1 and g.h % 2 == 0 and g.w % 2 == 0


def mirror_plan(g, cus=256, deep=True, splits=None):
    """wg_plan: what the launcher takes for g on `cus` compute units; splits: a forced split count (replaces cus / (grid y * tiles)
    before the clamps), None = nothing forced; deep: S2D_WG_RING_DEEP"""
    assert supported(g), g
    tco, tci = tile_of(g.cout), tile_of(g.cin)
    kxn = 2 if g.ks == 4 else g.ks
    gy = g.ks * (g.ks // kxn)
    tiles = (g.cout // tco) * (g.cin // tci)
    total = total_steps(g)
    want = splits if splits is not None else cus // (gy * tiles)
    want = max(1, min(want, total))
    spb = ceil_div(total, want)
    return Plan(tco, tci, cfg(tco, tci, g.ks, stride_of(g), deep).ns, kxn, ceil_div(total, spb), spb, gy, tiles)


def ws_floats(g, plan, with_rows=True):
    """the workspace: [splits][ks * ks][cout][cin] slabs, then [splits][cout] bias-gradient rows (always part of the queried size)"""
    return plan.splits * g.ks * g.ks * g.cout * g.cin + (plan.splits * g.cout if with_rows else 0)


def step_map(g, s):
    """K-step s -> (image, output row, 32-pixel column block)"""
    ho, wo = out_hw(g)
    xc_n = ceil_div(wo, 32)
    return s // (ho * xc_n), (s // xc_n) % ho, s % xc_n


def split_ranges(g, plan):
    total = total_steps(g)
    return [(k * plan.spb, min(total, (k + 1) * plan.spb)) for k in range(plan.splits)]


def boundary_kinds(g, plan):
    """where the splits after the first begin: {"mid-row", "mid-image", "image"} (row starts inside an image count as mid-image)"""
    ho, wo = out_hw(g)
    xc_n = ceil_div(wo, 32)
    kinds = set()
    for s0, _ in split_ranges(g, plan)[1:]:
        if s0 % xc_n:
            kinds.add("mid-row")
        elif s0 % (ho * xc_n):
            kinds.add("mid-image")
        else:
            kinds.add("image")
    return kinds


# ---- operands and references ------------------------------------------------------------------------------------------------------------
def int_operands(g, seed):
    """x [n, cin, h, w], dy [n, cout, Ho, Wo] float64: integers in {-3..3}, uniform"""
    ho, wo = out_hw(g)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (g.n, g.cin, g.h, g.w), generator=gen).double()
    dy = torch.randint(-3, 4, (g.n, g.cout, ho, wo), generator=gen).double()
    return x, dy


def wgrad64(g, x, dy):
    """float64 weight gradient by autograd -> [cout, cin, ks, ks]; ks 4: the ConvTranspose2d(4, 2, 1) whose input is dy's tensor"""
    x, dy = x.double(), dy.double()
    w = torch.zeros(g.cout, g.cin, g.ks, g.ks, dtype=torch.float64, requires_grad=True)
    if g.kind == S2 and g.ks == 4:
        y = F.conv_transpose2d(dy, w, None, stride=2, padding=1)
        assert y.shape == x.shape
        y.backward(x)
    else:
        y = F.conv2d(x, w, None, stride=stride_of(g), padding=g.pad)
        assert y.shape == dy.shape, (tuple(y.shape), tuple(dy.shape))
        y.backward(dy)
    return w.grad.detach()


def to_int(v):
    r = v.round().long()
    assert torch.equal(r.double(), v)
    return r


def reference(g, x, dy):
    """-> (dW int64 [cout, cin, ks, ks], dbias int64 [cout])"""
    return to_int(wgrad64(g, x, dy)), to_int(dy.sum((0, 2, 3)))


def assert_exact_condition(g, ref, what=""):
    """the one condition of the exact comparison, on the geometry and the reference alone"""
    ho, wo = out_hw(g)
    assert 9 * g.n * ho * wo < 2 ** 24, f"{what}: 9 * {g.n} * {ho} * {wo} >= 2^24: shrink the map (never the comparison)"
    top = int(ref.abs().max())
    assert top < 2 ** 24, what
    return top


def slab_references(g, plan, x, dy):
    """-> (slabs int64 [splits, ks, ks, cout, cin], rows int64 [splits, cout]): the contraction over each split's own output pixels"""
    ho, wo = out_hw(g)
    xc_n = ceil_div(wo, 32)
    cols = F.unfold(x.double(), g.ks, padding=g.pad, stride=stride_of(g))           # [n, cin ks ks, Ho Wo]
    assert cols.shape[2] == ho * wo
    cols = cols.permute(1, 0, 2).reshape(g.cin * g.ks * g.ks, -1)
    a = dy.double().reshape(g.n, g.cout, ho * wo).permute(1, 0, 2).reshape(g.cout, -1)
    img, yy, xx = torch.meshgrid(torch.arange(g.n), torch.arange(ho), torch.arange(wo), indexing="ij")
    split = (((img * ho + yy) * xc_n + xx // 32) // plan.spb).reshape(-1)
    assert int(split.max()) == plan.splits - 1
    slabs, rows = [], []
    for k in range(plan.splits):
        ix = (split == k).nonzero().flatten()
        s = a[:, ix] @ cols[:, ix].t()                                             # [cout, cin ks ks]
        slabs.append(s.reshape(g.cout, g.cin, g.ks, g.ks).permute(2, 3, 0, 1))
        rows.append(a[:, ix].sum(1))
    return to_int(torch.stack(slabs)), to_int(torch.stack(rows))


def nhwc_flat(t):
    """[n, c, h, w] -> the flat NHWC element order"""
    return t.permute(0, 2, 3, 1).reshape(-1).contiguous()


def fences(g):
    """elements of NaN on each side of (x, dY)"""
    return (g.w + 3) * g.cin, 33 * g.cout


def fenced(flat, front, dtype, device):
    """flat in the middle of a NaN-filled 1-D allocation -> (allocation, its body view)"""
    buf = torch.full((flat.numel() + 2 * front,), float("nan"), dtype=dtype, device=device)
    buf[front:front + flat.numel()] = flat.to(device=device, dtype=dtype)
    return buf, buf[front:front + flat.numel()]


def out_buffers(g, plan, with_db, device, ws_elems=None):
    """NaN-filled, guarded (dweight, dbias | None, workspace of exactly the plan's size) -> ((allocation, body), ...)"""
    dw = R.poisoned(g.cout, g.cin * g.ks * g.ks, dtype=torch.float32, device=device)
    db = R.poisoned(g.cout // 64, 64, dtype=torch.float32, device=device) if with_db else (None, None)
    n = ws_floats(g, plan) if ws_elems is None else ws_elems
    assert n % 64 == 0
    ws = R.poisoned(n // 64, 64, dtype=torch.float32, device=device)
    return dw, db, ws


# ---- checkers -----------------------------------------------------------------------------------------------------------------------------
def _first(bad):
    return bad.nonzero()[:8].tolist()


def _equal(got, want, what, names):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want.double()):
        bad = ~(got == want.double())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values differ from the exact reference ({int(torch.isnan(got).sum())} NaN); "
                             f"first ({names}): {_first(bad)}")


def check_case(g, plan, x, dy, dwbuf, dbbuf, wsbuf, what=""):
    """every check of one launch.  x, dy: the float64 operands; dwbuf / dbbuf / wsbuf: the `poisoned` allocations the launch wrote
    (dbbuf None: no bias gradient asked for).  -> max|dW ref|"""
    ref, ref_db = reference(g, x, dy)
    top = assert_exact_condition(g, ref, what)
    R.assert_written(dwbuf, what + " dweight")
    _equal(dwbuf[R.GUARD:-R.GUARD].reshape(g.cout, g.cin, g.ks, g.ks), ref, what + " dweight", "co, ci, ky, kx")
    slabs, rows = slab_references(g, plan, x, dy)
    assert torch.equal(slabs.sum(0).permute(2, 3, 0, 1), ref), "the split references do not add up to the autograd reference"
    R.assert_guards(wsbuf, what + " workspace")
    ws = wsbuf[R.GUARD:-R.GUARD].reshape(-1)
    n_slab = ws_floats(g, plan, with_rows=False)
    assert ws.numel() == ws_floats(g, plan), (what, "workspace size", ws.numel(), ws_floats(g, plan))
    _equal(ws[:n_slab].reshape(slabs.shape), slabs, what + " per-split slabs", "split, ky, kx, co, ci")
    if dbbuf is None:
        R.assert_untouched(ws[n_slab:], what + " workspace rows behind the slabs (no bias gradient asked for)")
    else:
        _equal(ws[n_slab:].reshape(rows.shape), rows, what + " per-split bias-gradient rows", "split, co")
        R.assert_written(dbbuf, what + " dbias")
        _equal(dbbuf[R.GUARD:-R.GUARD].reshape(-1), ref_db, what + " dbias", "co")
    return top


def old_criterion(dw, ref, tol):
    """the criterion of tests/test_dense2d_gpu.py (1e-3) / test_conv_s2_gpu.py (2e-3): max|dW - ref| <= tol * max|ref|"""
    return bool((dw.double() - ref.double()).abs().max() <= tol * ref.double().abs().max())


# ---- host emulation of the launch (plain torch, fp32 accumulate) ------------------------------------------------------------------------
DEFECTS = ("last_step_dropped", "step_twice", "stale_slot", "kx_off", "pad_column", "outside_row", "filler", "s2_stride1", "cot_cit_swapped",
           "split_left_out", "dbias_cit1", "row_past_cout")


def _body(buf):
    """a `poisoned` allocation -> (its flat view, the offset of the body's first element)"""
    return buf.reshape(-1), R.GUARD * (buf.numel() // buf.shape[0])


def emulate(g, plan, xbuf, fx, dybuf, fd, dwbuf, dbbuf, wsbuf, defect=None):
    """The launch on the host.  Workgroup (split, ky / kx group, co tile x ci tile) walks its K-steps with the incremental (n, y, xc)
    counter, stages dY[32 px][TCO] and X[31 stride + ks px][TCI] of input row y stride + ky - pad through an NS-slot ring (range tests
    against Wo / W, a kernel row outside the image and the pad columns read the zero page), takes tap kx as a row offset of the X tile
    (row stride = the conv stride), accumulates in fp32, stores its [kx][co][ci] slabs and, for ky group 0 / ci tile 0, the per-channel
    sums of its dY tiles; then the four-row fixed-order fold into dW [cout][cin][ks][ks] and dbias.
    xbuf / dybuf: fenced 1-D fp32 allocations whose tensor starts at element fx / fd (a fetch that misses its range test reads what lies
    there: a neighbouring pixel row, image, or the NaN fence); dwbuf / dbbuf / wsbuf: `poisoned` allocations.  defect: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    ks, st, taps = g.ks, stride_of(g), g.ks * g.ks
    ho, wo = out_hw(g)
    xc_n, total = ceil_div(wo, 32), total_steps(g)
    tco, tci, ns, kxn = plan.tco, plan.tci, plan.ns, plan.kxn
    kxg, cot_n, cit_n = ks // kxn, g.cout // plan.tco, g.cin // plan.tci
    assert plan.gy == ks * kxg and plan.gz == cot_n * cit_n
    nbv = 31 * st + ks                                   # rows of the X tile that can be in range
    ws, wso = _body(wsbuf)
    dbp0 = wso + plan.splits * taps * g.cout * g.cin     # [splits][cout] behind the slabs
    zero = torch.zeros(())
    ra, rb = torch.arange(32), torch.arange(nbv)
    ca, cb = torch.arange(tco), torch.arange(tci)
    db_rows = {}
    for bx in range(plan.splits):
        s0, s1 = bx * plan.spb, min(total, (bx + 1) * plan.spb)
        if defect == "last_step_dropped" and bx == plan.splits - 1:
            s1 -= 1
        if defect == "step_twice" and bx == 1:
            s0 -= 1
        n = s1 - s0
        for by in range(plan.gy):
            ky, kx0 = by // kxg, (by % kxg) * kxn
            for bz in range(plan.gz):
                cot, cit = bz // cit_n, bz % cit_n
                if defect == "cot_cit_swapped":            # the two tile counts exchanged in the decode (a bijection only if they are equal)
                    cot, cit = bz // cot_n, bz % cot_n
                state = {"sn": s0 // (ho * xc_n), "sy": (s0 // xc_n) % ho, "sxc": s0 % xc_n}
                slots = [None] * ns

                def stage(slot):
                    sn, sy, sxc = state["sn"], state["sy"], state["sxc"]
                    x0, yin = sxc * 32, sy * st + ky - g.pad
                    ua = ((sn * ho + sy) * wo + x0) * g.cout
                    ub = ((sn * g.h + yin) * g.w + x0 * st - g.pad) * g.cin
                    lim_b = g.w if (0 <= yin < g.h or defect == "outside_row") else 0
                    ok_a = (x0 + ra) < wo
                    if defect == "filler":
                        ok_a = torch.ones_like(ok_a)
                    xv = x0 * st - g.pad + rb
                    ok_b = (xv >= 0) & (xv < lim_b)
                    if defect == "pad_column" and lim_b:
                        ok_b = (xv >= -1) & (xv <= lim_b)
                    ia = (fd + ua + ra[:, None] * g.cout + cot * tco + ca[None]).clamp(0, dybuf.numel() - 1)
                    ib = (fx + ub + rb[:, None] * g.cin + cit * tci + cb[None]).clamp(0, xbuf.numel() - 1)
                    a = torch.where(ok_a[:, None], dybuf[ia], zero)
                    b = torch.where(ok_b[:, None], xbuf[ib], zero)
                    slots[slot] = (a, torch.cat([b, torch.zeros(1, tci)]))
                    state["sxc"] += 1                      # advance()
                    if state["sxc"] == xc_n:
                        state["sxc"] = 0
                        state["sy"] += 1
                        if state["sy"] == ho:
                            state["sy"] = 0
                            state["sn"] += 1

                acc = torch.zeros(kxn, tco, tci)
                dbs = torch.zeros(tco)
                do_db = dbbuf is not None and by == 0 and (cit == 0 or (defect == "dbias_cit1" and cit == 1))
                for j in range(min(ns - 1, n)):
                    stage(j)
                for i in range(n):
                    if i + ns - 1 < n:
                        if defect == "stale_slot" and i + ns - 1 == ns:
                            state_before = dict(state)
                            keep = slots[(i + ns - 1) % ns]
                            stage((i + ns - 1) % ns)               # the counter advances, the slot keeps step i - 1's tiles
                            slots[(i + ns - 1) % ns] = keep
                            assert state_before != state
                        else:
                            stage((i + ns - 1) % ns)
                    a, b = slots[i % ns]
                    if do_db:
                        dbs += a.sum(0)
                    for kx in range(kxn):
                        rows = ra * (1 if defect == "s2_stride1" else st) + kx0 + kx
                        if defect == "kx_off" and kx0 + kx == 1:
                            rows = rows + 1
                        acc[kx] += a.t() @ b[rows]
                if do_db:
                    key = (bx, cot)
                    db_rows[key] = db_rows.get(key, 0) + dbs
                for kx in range(kxn):
                    base = wso + ((bx * taps + ky * ks + kx0 + kx) * g.cout + cot * tco) * g.cin + cit * tci
                    assert 0 <= base and base + (tco - 1) * g.cin + tci <= ws.numel(), "a slab store outside the workspace allocation"
                    ws[base + ca[:, None] * g.cin + cb[None]] = acc[kx]
                    if defect == "row_past_cout" and bx == plan.splits - 1 and ky * ks + kx0 + kx == taps - 1 and cot == cot_n - 1:
                        assert base + tco * g.cin + tci <= ws.numel(), "a slab store outside the workspace allocation"
                        ws[base + tco * g.cin + cb] = acc[kx][-1]
    for (bx, cot), v in db_rows.items():
        ws[dbp0 + bx * g.cout + cot * tco + ca] = v
    # conv3x3_wgrad_reduce_kernel: thread row sl folds splits sl, sl + 4, ...; the four rows are added in a fixed order
    n_fold = plan.splits - 1 if defect == "split_left_out" else plan.splits
    size = taps * g.cout * g.cin

    def fold(off, width):
        rows = []
        for sl in range(4):
            s = torch.zeros(width)
            for k in range(sl, n_fold, 4):
                s = s + ws[off + k * width:off + (k + 1) * width]
            rows.append(s)
        return rows
    r = fold(wso, size)
    t = ((r[0] + r[1]) + r[2]) + r[3]
    dw, dwo = _body(dwbuf)
    dw[dwo:dwo + size] = t.reshape(taps, g.cout * g.cin).t().reshape(-1)      # dw[(co cin + ci) taps + tap]
    if dbbuf is not None:
        r = fold(dbp0, g.cout)
        db, dbo = _body(dbbuf)
        db[dbo:dbo + g.cout] = (r[0] + r[1]) + (r[2] + r[3])


def plan_line(tag, g, plan, deep, top=None):
    ho, wo = out_hw(g)
    return (f"{tag:<40} {ENTRY_NAMES[entry_of(g)]:<7} {g.n}x{g.h}x{g.w} (out {ho}x{wo}) {g.cin}->{g.cout} p{g.pad}: TCO {plan.tco}, TCI {plan.tci}, "
            f"ring {'deep' if deep else 'four-slot'} NS {plan.ns}, KXN {plan.kxn}, splits {plan.splits} x {plan.spb} steps of {total_steps(g)}, "
            f"grid {plan.splits}x{plan.gy}x{plan.gz}" + ("" if top is None else f", max|ref| {top}"))
