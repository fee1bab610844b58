"""TEST INFRASTRUCTURE ONLY - exact references, a launch-plan mirror, checkers and a host emulation for the dense 2-D tile kernels of
csrc/conv2d_nhwc.hip (s2d_conv2d3x3 / 1x1 / 4x4s2 / 2x2s2 and s2d_convup, with their statistics and batch-norm-backward epilogues).
Imports without a GPU and never loads the native library: tests/test_conv2d_parity_gpu.py drives the entries,
tests/test_conv2d_checks_cpu.py shows on the host that every checker below can fail.

Method.  Nothing below is fitted to what the kernels return.
  exact set: activations, weights and bias are small integers (exact in bf16), the reference is torch's conv2d / conv_transpose2d in
      float64 on the host (exact at these magnitudes) cast to int64.  The condition asserted ON THE REFERENCE ALONE is
      max|ref| <= 256 (EXACT_MAX): every output is then a bf16 value (8 significant bits cover the integers up to 256), every partial
      sum of the fp32 accumulation is an integer below 2^24 whatever the order, so y is compared with torch.equal.  The per-tile
      statistics slabs are exact too: |sum| <= 128 * 256, sum of squares <= 128 * 2^16 = 2^23, compared with torch.equal against
      int64 sums over each tile's own rows (membership from the plan report).
  rounding set: {-3..3} operands, sums run past 256, odd integers in (256, 512) are exact bf16 ties.  Reference: int64 -> float32 ->
      bfloat16 by torch on the host (round to nearest even), compared on the bits.  The sum slab stays exact (integers, |sum| < 2^24);
      the sum-of-squares slab is compared with the float64 sum of the stored values under the forward bound of recursive summation
      for the epilogue's chain: 4 MI adds per lane (the squares of bf16 values are exact in fp32), two shuffles, one LDS add ->
      L = 4 MI + 3 (check_sums of bn_pass_ref.py).
  batch-norm-backward epilogue: z in {-3..3} (even in the channels whose |scale| is 0.5), scale in {+-0.5, +-1, +-2}, shift an integer
      + 0.5: pre = z scale + shift is exact in fp32 and never 0 (asserted).  act 0 / 1: g is dy or 0, both slabs are exact integers
      (|sum g z| <= 128 * 768) -> torch.equal.  act 2: float64 dy gelu'(pre) sums; bound = the activation term
      E_ACT max(1, |pre|) |dy| of bn_pass_ref.py (measured against float64 with a factor 4, profiles/bn_pass_parity.txt) + the chain
      bound with L = 4 MI + 3 + 2 (the two extra for the roundings of the products dy * gelu' and g * z, which are not exact here).
  fencing: x sits in the middle of a NaN-filled allocation with (W + 3) * cin elements on each side, so an out-of-image fetch the
      zero page does not replace is a NaN in y; y and the slabs are exact-size, NaN-filled, with guard rows (poisoned /
      assert_written of bn_pass_ref.py): every element written, every guard intact.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import bn_pass_ref as R

K3, K3_BNBWD, K1, K1_BNBWD, UP, K4S2, K2S2 = range(7)
KIND_NAMES = ("3x3", "3x3 bnbwd", "1x1", "1x1 bnbwd", "up", "4x4s2", "2x2s2")
K32, K64, SHARED_A = 0, 1, 2
FAMILY_NAMES = ("k32", "64-deep ring", "shared-A")
EXACT_MAX = 256
BF = torch.bfloat16

Plan = namedtuple("Plan", "family bn rows ns gx gy gz tiles")
Geo = namedtuple("Geo", "kind n h w cin cout pad stride ks")


def geo(kind, n, h, w, cin, cout, pad=None, stride=None, ks=None):
    """the entry's own arguments; pad / stride / ks filled in for the kinds that fix them"""
    fixed = {K1: (0, 1, 1), K1_BNBWD: (0, 1, 1), K4S2: (1, 2, 4), K2S2: (0, 2, 2)}
    if kind in fixed:
        pad, stride, ks = fixed[kind]
    elif kind == UP:
        pad, stride = 1, 2
    else:
        ks = 3
    return Geo(kind, n, h, w, cin, cout, pad, stride, ks)


def ceil_div(a, b):
    return -(-a // b)


def gemm_hw(g):
    """the grid of the implicit GEMM's rows: the output image, for UP the source grid (one GEMM per parity class)"""
    if g.kind in (K3, K3_BNBWD):
        return (g.h + 2 * g.pad - 3) // g.stride + 1, (g.w + 2 * g.pad - 3) // g.stride + 1
    if g.kind in (K4S2, K2S2):
        return g.h // 2, g.w // 2
    return g.h, g.w


def gemm_rows(g):
    ho, wo = gemm_hw(g)
    return g.n * ho * wo


def out_pixels(g):
    return (4 if g.kind == UP else 1) * gemm_rows(g)


def mi_of(plan):
    return plan.rows // 32


# ---- the parent commit's launch arithmetic, restated (no switch set, `cus` compute units) --------------------------------------------
def conv_bn(cout):
    return 128 if cout % 128 == 0 else 64


def k32_rows(m, col_blocks, cus=256):
    """conv_k32_rows: cost = max(workgroups, 3 * CUs) * (rows + 48), tried in the order 128, 96, 64, the first strict minimum wins"""
    slots = 3 * cus
    best, best_cost = 128, None
    for bm in (128, 96, 64):
        blocks = ceil_div(m, bm) * col_blocks
        cost = max(blocks, slots) * (bm + 48)
        if best_cost is None or cost < best_cost:
            best, best_cost = bm, cost
    return best


def mirror_plan(g, cus=256):
    """what the parent commit launches for g with no switch set: conv_use_shared_a (pad 1, stride 1, 64-wide column blocks, cin >= 128),
    conv_tile_rows / convup_rows (4 m) / conv1x1_rows (k32 rows only at 128-wide blocks), conv1x1_use_k32 (cin >= 128), the 2x2 stride-2
    conv always on the 64-deep double buffer, grids xcd_grid(row tiles) x cout / BN [x 4 classes]"""
    m, bn = gemm_rows(g), conv_bn(g.cout)
    cb = g.cout // bn
    family, rows, ns = K32, 128, 3
    if g.kind in (K3, K3_BNBWD) and g.pad == 1 and g.stride == 1 and bn == 64 and g.cin >= 128:
        family, ns = SHARED_A, 2
    elif g.kind in (K1, K1_BNBWD) and g.cin < 128:
        family, ns = K64, 2
    elif g.kind == K2S2:
        family, ns = K64, 2
    if family == K32 and bn == 128:
        rows = k32_rows(4 * m if g.kind == UP else m, cb, cus)
    row_tiles = ceil_div(m, rows)
    gz = 4 if g.kind == UP else 1
    return Plan(family, bn, rows, ns, ceil_div(row_tiles, 8) * 8, cb, gz, gz * row_tiles)


# ---- operands and references ------------------------------------------------------------------------------------------------------------
def weight_shape(g):
    if g.kind == UP:
        return (g.cin, g.cout, g.ks, g.ks)       # ConvTranspose2d layout [K channels][N channels][ks][ks]
    return (g.cout, g.cin, g.ks, g.ks)


def int_operands(g, amp, seed, bias):
    """x [n, cin, h, w] float64, weight float32 in the entry's layout, bias float32 | None: integers in [-amp, amp], uniform"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-amp, amp + 1, (g.n, g.cin, g.h, g.w), generator=gen).double()
    w = torch.randint(-amp, amp + 1, weight_shape(g), generator=gen).float()
    b = torch.randint(-2, 3, (g.cout,), generator=gen).float() if bias else None
    return x, w, b


def conv64(g, x, w, b):
    """the float64 convolution of the entry on the host -> [out pixels, cout] float64 in NHWC row order"""
    x, w = x.double(), w.double()
    b = None if b is None else b.double()
    if g.kind == UP:
        y = F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1 if g.ks == 3 else 0)
        assert y.shape[2:] == (2 * g.h, 2 * g.w)
    else:
        y = F.conv2d(x, w, b, stride=g.stride, padding=g.pad)
        assert tuple(y.shape[2:]) == gemm_hw(g), (tuple(y.shape), gemm_hw(g))
    return y.permute(0, 2, 3, 1).reshape(-1, g.cout).contiguous()


def reference(g, x, w, b):
    """-> int64 [out pixels, cout] (the float64 convolution of integer operands is exact)"""
    y = conv64(g, x, w, b)
    r = y.round().long()
    assert torch.equal(r.double(), y)
    return r


def assert_exact_condition(ref, what=""):
    """the one condition of the exact set, asserted on the reference alone"""
    top = int(ref.abs().max())
    assert top <= EXACT_MAX, f"{what}: max|ref| = {top} > {EXACT_MAX}: change the seed or thin the operands (never the comparison)"
    return top


def nhwc_rows(x):
    """[n, c, h, w] -> [n h w, c]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def fence_rows(g):
    """rows (pixels) of NaN on each side of x: (W + 3) pixels = (W + 3) * cin elements"""
    return g.w + 3


def fenced(rows, front, dtype, device):
    """rows [m, c] in the middle of a NaN-filled [front + m + front, c] allocation -> (allocation, its body view)"""
    buf = torch.full((rows.shape[0] + 2 * front, rows.shape[1]), float("nan"), dtype=dtype, device=device)
    buf[front:front + rows.shape[0]] = rows.to(device=device, dtype=dtype)
    return buf, buf[front:front + rows.shape[0]]


# ---- tiles ----------------------------------------------------------------------------------------------------------------------------------
def up_out_index(g, m, p, q):
    """row m = (img, i, j) of the source grid -> the output pixel (img, 2 i + p, 2 j + q) of the [2h][2w] image"""
    j, t = m % g.w, m // g.w
    i, img = t % g.h, t // g.h
    return ((img * 2 * g.h) + 2 * i + p) * (2 * g.w) + 2 * j + q


def slab_members(g, plan):
    """per statistics slab, the output pixels (row indices of y) it sums; UP: slab = class * ceil(m / rows) + tile"""
    m = gemm_rows(g)
    row_tiles = ceil_div(m, plan.rows)
    members = []
    for cls in range(4 if g.kind == UP else 1):
        for t in range(row_tiles):
            ms = torch.arange(t * plan.rows, min((t + 1) * plan.rows, m))
            members.append(up_out_index(g, ms, cls >> 1, cls & 1) if g.kind == UP else ms)
    assert len(members) == plan.tiles, (len(members), plan.tiles)
    return members


def slab_sums(a, b, members):
    """-> [tiles, 2, c]: (sum a, sum a * b) over each slab's rows, in the dtype of a (int64 or float64)"""
    return torch.stack([torch.stack([a[ix].sum(0), (a[ix] * b[ix]).sum(0)]) for ix in members])


# ---- checkers -----------------------------------------------------------------------------------------------------------------------------
def _first(bad):
    return bad.nonzero()[:8].tolist()


def check_y_exact(y, ref, what="y"):
    """y (bf16 [out pixels, cout]) == ref (int64) with torch.equal, under max|ref| <= 256"""
    assert_exact_condition(ref, what)
    got = y.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if not torch.equal(got, ref.double()):
        bad = ~(got == ref.double())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ from the exact reference ({int(torch.isnan(got).sum())} "
                             f"NaN); first (pixel, channel): {_first(bad)}")


def rounded(ref):
    """int64 -> float32 -> bfloat16 by torch on the host: round to nearest even"""
    assert int(ref.abs().max()) < 2 ** 24
    return ref.float().to(BF)


def check_y_rounded(y, ref, what="y"):
    """the bits of y == the bits of rounded(ref)"""
    got, want = y.detach().cpu().contiguous(), rounded(ref)
    assert got.shape == want.shape and got.dtype == BF, (what, tuple(got.shape), got.dtype)
    if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        bad = got.view(torch.int16) != want.view(torch.int16)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ in their bits from round-to-nearest-even of the exact "
                             f"reference ({int(torch.isnan(got).sum())} NaN); first (pixel, channel): {_first(bad)}")


def check_slabs_exact(slabs, stored, members, what="slabs"):
    """slabs [tiles, 2, c] fp32 == int64 (sum, sum of squares) of the stored outputs over each tile's own rows (torch.equal)"""
    want = slab_sums(stored, stored, members)
    assert int(want.abs().max()) < 2 ** 24
    got = slabs.detach().double().cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want.double()):
        bad = ~(got == want.double())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} slab sums differ from the exact tile sums; first (slab, which, channel): "
                             f"{_first(bad)}")


def check_slabs_rounded(slabs, y, members, mi, what="slabs", family=None):
    """rounding set: the sum slab == the exact sum of the STORED values, the sum-of-squares slab within (4 MI + 3) 2^-24 sum y^2"""
    stored = y.detach().double().cpu()
    want = slab_sums(stored, stored, members)
    assert float(want[:, 0].abs().max()) < 2 ** 24 and torch.equal(want[:, 0], want[:, 0].round())
    got = slabs.detach().double().cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got[:, 0], want[:, 0]):
        bad = ~(got[:, 0] == want[:, 0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} sums differ from the exact sums of the stored outputs; first (slab, channel): "
                             f"{_first(bad)}")
    R.check_sums(got[:, 1].flatten(), want[:, 1].flatten(), want[:, 1].flatten(), 4 * mi + 3, what=what + " (sum of squares)", family=family)


def bnbwd_operands(m, c, seed):
    """z [m, c] (bf16-exact integers), scale, shift [c] of the batch norm whose output gradient the conv produces"""
    gen = torch.Generator().manual_seed(seed)
    scale = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[torch.randint(0, 6, (c,), generator=gen)]
    shift = torch.randint(-3, 3, (c,), generator=gen).float() + 0.5
    z = torch.randint(-3, 4, (m, c), generator=gen).float()
    half = scale.abs() == 0.5
    z[:, half] = 2.0 * torch.randint(-1, 2, (m, int(half.sum())), generator=gen).float()   # keeps pre off 0 where |scale| = 0.5
    pre = z.double() * scale.double() + shift.double()
    assert bool((pre != 0).all())
    return z, scale, shift


def check_slabs_bnbwd(slabs, y, z, scale, shift, act, members, mi, what="bnbwd slabs", family=None):
    """slabs = per-tile (sum g, sum g z), g = dy act'(z scale + shift) over the STORED dy = y.  act 0 / 1: torch.equal against the exact
    integer sums; act 2: float64 sums, bound = summed activation terms + (4 MI + 5) 2^-24 sum|term|"""
    dy, zz = y.detach().double().cpu(), z.double()
    pre = zz * scale.double() + shift.double()
    assert bool((pre != 0).all())
    g, g_err = R.ref_g(dy, act, z=pre)
    got = slabs.detach().double().cpu()
    assert got.shape == (len(members), 2, dy.shape[1]), (what, tuple(got.shape))
    if act in (0, 1):
        want = slab_sums(g, zz, members)
        assert float(want.abs().max()) < 2 ** 24 and torch.equal(want, want.round())
        if not torch.equal(got, want):
            bad = ~(got == want)
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} backward sums differ from the exact tile sums; first "
                                 f"(slab, which, channel): {_first(bad)}")
        return
    for t, ix in enumerate(members):
        ref, mag, act_term = R.ref_bwd_sums(g[ix], g_err[ix], zz[ix])
        R.check_sums(got[t].flatten(), ref, mag, 4 * mi + 5, act_term, what=f"{what} (slab {t})", family=family)


def check_case(g, plan, mode, ref, ybuf, slabbuf=None, bnbwd=None, what="", family=None):
    """every check of one launch: ybuf / slabbuf are `poisoned` allocations the launch wrote (guards intact, every element written),
    mode "exact" (torch.equal under max|ref| <= 256) or "rounded" (bit-equal to round-to-nearest-even; bounded sum of squares),
    bnbwd = (z, scale, shift, act) where the slabs are the batch-norm backward sums"""
    assert mode in ("exact", "rounded")
    R.assert_written(ybuf, what + " y")
    y = ybuf[R.GUARD:-R.GUARD]
    if mode == "exact":
        check_y_exact(y, ref, what + " y")
    else:
        check_y_rounded(y, ref, what + " y")
    if slabbuf is None:
        return
    R.assert_written(slabbuf, what + " slabs")
    slabs, members = slabbuf[R.GUARD:-R.GUARD], slab_members(g, plan)
    if bnbwd is not None:
        z, scale, shift, act = bnbwd
        check_slabs_bnbwd(slabs, y, z, scale, shift, act, members, mi_of(plan), what + " bnbwd slabs", family)
    elif mode == "exact":
        check_slabs_exact(slabs, ref, members, what + " slabs")
    else:
        check_slabs_rounded(slabs, y, members, mi_of(plan), what + " slabs", family)


def old_criterion(out, ref):
    """the criterion of tests/test_dense2d_gpu.py / test_conv_s2_gpu.py (6e-3 * max|ref|), kept to show what it lets through"""
    return bool(((out.double() - ref.double()).abs().max() <= 6e-3 * ref.double().abs().max()))


def old_stats_criterion(slabs, y):
    """the old statistics check: the slabs summed over all tiles against column sums of the stored output at 1e-3 * max + 1e-2"""
    yf = y.double()
    s1, s2 = yf.sum(0), (yf * yf).sum(0)
    p = slabs.double().sum(0)
    return bool((p[0] - s1).abs().max() <= 1e-3 * s1.abs().max() + 1e-2) and bool((p[1] - s2).abs().max() <= 1e-3 * s2.abs().max())


# ---- host emulation of the tiling (plain torch, fp32 accumulate) ------------------------------------------------------------------------
DEFECTS = ("border_tap", "edge_wrap", "straddle", "substep_dropped", "substep_twice", "truncate", "slab_unrounded", "slab_index",
           "row_past_end", "class_swap")


def _class_taps(g, w, cls):
    """-> (base offset of the window's corner pixel (by, bx) relative to stride * (oy, ox), [(dy, dx, B [K, N])]) of one parity class"""
    if g.kind != UP:
        return (-g.pad, -g.pad), [(ky, kx, w[:, :, ky, kx].t().contiguous()) for ky in range(g.ks) for kx in range(g.ks)]
    p, q = cls >> 1, cls & 1
    ty_n, tx_n = (g.ks + p) // 2, (g.ks + q) // 2
    taps = [(ty, tx, w[:, :, 2 * (ty_n - 1 - ty) + 1 - p, 2 * (tx_n - 1 - tx) + 1 - q].contiguous()) for ty in range(ty_n) for tx in range(tx_n)]
    return (p - (ty_n - 1), q - (tx_n - 1)), taps


def truncate_bf16(v):
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def emulate(g, rows, xbuf, front, w, b, ybuf, slabbuf=None, defect=None, bnbwd=None):
    """The tile kernels on the host: loops over parity classes, row tiles, taps and 32-channel sub-steps, fp32 accumulate, one bf16 store,
    per-tile slabs, the UP scatter.  xbuf = the fenced allocation [front + n h w + front, cin] (a fetch that misses its mask reads what
    lies there: a neighbouring row, image, or the NaN fence); ybuf / slabbuf = `poisoned` allocations (with their guard rows).
    defect = one of DEFECTS; bnbwd = (z, scale, shift, act)."""
    assert defect is None or defect in DEFECTS
    m_total = gemm_rows(g)
    ho, wo = gemm_hw(g)
    stride = 1 if g.kind == UP else g.stride
    row_tiles = ceil_div(m_total, rows)
    xf, wf = xbuf.float(), w.to(BF).float()
    last = xf.shape[0] - 1
    hit_tile = row_tiles - 1
    for cls in range(4 if g.kind == UP else 1):
        (by, bx), taps = _class_taps(g, wf, cls)
        p, q = cls >> 1, cls & 1
        if defect == "class_swap" and cls in (1, 2):
            p, q = q, p
        for t in range(row_tiles):
            ms = torch.arange(t * rows, (t + 1) * rows)
            valid = ms < m_total
            mm = torch.where(valid, ms, torch.zeros_like(ms))
            ox, oy, img = mm % wo, (mm // wo) % ho, mm // (wo * ho)
            if defect == "straddle":
                img = torch.full_like(img, int(img[0]))
            acc = torch.zeros(rows, g.cout)
            for ti, (dy, dx, bmat) in enumerate(taps):
                iy, ix = oy * stride + by + dy, ox * stride + bx + dx
                ok_y, ok_x = (iy >= 0) & (iy < g.h), (ix >= 0) & (ix < g.w)
                if defect == "border_tap" and dy == 0 and dx == 1:
                    ok_y = torch.ones_like(ok_y)
                if defect == "edge_wrap" and dx == 0:
                    ok_x = torch.ones_like(ok_x)
                ok = valid & ok_y & ok_x
                a = torch.where(ok[:, None], xf[(front + (img * g.h + iy) * g.w + ix).clamp(0, last)], torch.zeros(()))
                for sub in range(g.cin // 32):
                    reps = 1
                    if t == hit_tile and ti == len(taps) - 1 and sub == g.cin // 32 - 1:
                        reps = 0 if defect == "substep_dropped" else 2 if defect == "substep_twice" else 1
                    for _ in range(reps):
                        acc += a[:, 32 * sub:32 * sub + 32] @ bmat[32 * sub:32 * sub + 32]
            v = acc + (b if b is not None else 0.0)
            stored = truncate_bf16(v) if defect == "truncate" else v.to(BF)
            mo = up_out_index(g, mm, p, q) if g.kind == UP else mm
            ybuf[R.GUARD + mo[valid]] = stored[valid]
            if defect == "row_past_end" and t == row_tiles - 1 and cls == 0:
                ybuf[R.GUARD + out_pixels(g)] = stored[-1]
            if slabbuf is not None:
                src = (v if defect == "slab_unrounded" else stored.float())[valid]
                if bnbwd is not None:
                    z, scale, shift, act = bnbwd
                    zf = z.float()[mm[valid]]
                    gg = R.emu_g(src, zf, scale, shift, act)
                    s = torch.stack([gg.sum(0), (gg * zf).sum(0)])
                else:
                    s = torch.stack([src.sum(0), (src * src).sum(0)])
                slabbuf[R.GUARD + (t if defect == "slab_index" else cls * row_tiles + t)] = s


def emu_plan(g, rows=None):
    """a plan for the emulation: the mirror's, with another tile height where asked"""
    p = mirror_plan(g)
    if rows is None or rows == p.rows:
        return p
    row_tiles = ceil_div(gemm_rows(g), rows)
    return p._replace(rows=rows, gx=ceil_div(row_tiles, 8) * 8, tiles=p.gz * row_tiles)


def plan_line(tag, g, plan, top=None):
    return (f"{tag:<34} {KIND_NAMES[g.kind]:<9} {g.n}x{g.h}x{g.w} {g.cin}->{g.cout} p{g.pad} s{g.stride} k{g.ks}: {FAMILY_NAMES[plan.family]}, BN {plan.bn}, "
            f"rows {plan.rows}, NS {plan.ns}, grid {plan.gx}x{plan.gy}x{plan.gz}, tiles {plan.tiles}" + ("" if top is None else f", max|ref| {top}"))
