"""Shared by tests/test_spconv_wgrad_parity_gpu.py and tests/test_spconv_wgrad_checks_cpu.py: exact operands and reference of the sparse
weight gradient dW[k] = gather(feat, nbr[k])^T @ dout (csrc/spconv.hip), gather-map builders, a host restatement of the launch plan
(wgrad_plan, wgrad_block) and the launcher that runs a C-ABI entry into caller-owned, NaN-filled, fenced buffers.

Why exact: the operands are integers in {-3 .. 3}, stored as fp32 and as bf16 (the same values).  Every product is an integer of
magnitude <= 9 and every partial sum one below 9 * n_out < 2^24, so fp32 accumulation is exact in ANY order, over ANY row split, through
any MFMA shape, and the result is compared with torch.equal.  One missing, doubled, misplaced or (0, 0)-replaced pair changes cin * cout
sums by the products of its rows - invisible only if all of them vanish, which two seeds per case rule out.

Nothing here touches a GPU at import; run_entry and query_plan load the library when called.
"""
import ctypes
import functools

import torch

MFMA_CHANNELS = (16, 32, 64, 128)
SHAPES16 = [(ci, co) for ci in MFMA_CHANNELS for co in MFMA_CHANNELS]
VALU_SHAPES = [(5, 16, 27), (5, 3, 27), (24, 16, 27), (5, 4, 1), (3, 3, 3)]   # (cin, cout, kvol)
ENTRIES = {"f32": 0, "bf16": 1, "s16": 2}                                     # entry -> the mode wgrad_plan knows it by
KERNELS = ("mfma_f32", "bf16_reg", "tr", "coop128", "valu")                   # kernel id of s2d_spconv_wgrad_plan
HOOKS = ("S2D_WGRAD_TR", "S2D_WGRAD_COOP", "S2D_WGRAD_WAVES")
GRID_N_OUT = (1, 5, 255, 256, 257, 2000, 4097, 8300, 47890, 288892)           # the plan grid of the mirror / invariant tests
GRID_KVOL = (1, 8, 27)
BENCH_CASES = ((128, 128, 47890), (64, 64, 126079), (64, 128, 47890), (32, 32, 265026), (16, 16, 288892))   # (cin, cout, n_out) of the benchmark scene
MAX_ROWS = (1 << 24) // 9                                                     # exactness: 9 * n_out < 2^24


def ceil_div(a, b):
    return -(-a // b)


# ---- the launch plan, restated (csrc/spconv.hip: wgrad_plan, wgrad_block) ----------------------------------------------------------------
def mirror_plan(mode, n_out, kvol, cin, cout, tr=None, coop=None, waves=None):
    """what s2d_spconv_wgrad_plan answers; tr / coop / waves: the values of S2D_WGRAD_TR / _COOP / _WAVES, None = unset"""
    mfma = cin in MFMA_CHANNELS and cout in MFMA_CHANNELS
    tr_pref = 2 if tr is None else (1 if str(tr)[:1] == "1" else 0)
    is_tr = mode == 2 and mfma and (tr_pref == 1 or (tr_pref == 2 and cin <= 64))
    is_coop = mode == 2 and not is_tr and (1 if coop is None else int(coop)) != 0 and cin == 128 and cout in (64, 128)
    wco = cout // (16 * (2 if cout >= 32 else 1)) if mfma else 1
    if is_tr:
        wco = cout // (16 * min(cout // 16, 2 if cin == 128 else 4))
    wrow = 1 if is_coop or not mfma else 4 // wco
    want_waves = int(waves) if waves is not None and int(waves) > 0 else 2048
    blocks_y = max(1, want_waves // (kvol * 4))
    rows = max(n_out, 1)
    max_split = ceil_div(rows, 256)
    if is_tr and cin * cout <= 32 * 32:
        blocks_y *= 2
    if blocks_y * wrow > max_split:
        blocks_y = max(1, max_split // wrow)
    if is_tr and blocks_y >= 8:
        blocks_y &= ~7
    splits = ceil_div(min(blocks_y * wrow, max_split), wrow) * wrow
    kernel = 4 if not mfma else 3 if is_coop else 2 if is_tr else 0 if mode == 0 else 1
    return dict(kernel=kernel, n_split=splits, rows_per_split=ceil_div(ceil_div(rows, splits), 4) * 4, grid_y=splits // wrow, wrow=wrow)


def query_plan(mode, n_out, kvol, cin, cout):
    """s2d_spconv_wgrad_plan under the environment as it is now"""
    from sparse2dense_amd import _lib
    out = (ctypes.c_int32 * 5)()
    _lib.check(_lib.load().s2d_spconv_wgrad_plan(mode, int(n_out), kvol, cin, cout, out), "s2d_spconv_wgrad_plan")
    return dict(zip(("kernel", "n_split", "rows_per_split", "grid_y", "wrow"), (int(v) for v in out)))


def block_of(bx, by, kvol, grid_y, swapped=False):
    """wgrad_block: workgroup (bx, by) of a kvol x grid_y launch -> (kernel offset, row block); swapped: the two branches exchanged"""
    if (grid_y % 8 == 0) != swapped:
        b = bx + kvol * by
        return (b >> 3) % kvol, ((b >> 3) // kvol) * 8 + (b & 7)
    return bx, by


def empty_splits(plan, n_out):
    return sum(1 for s in range(plan["n_split"]) if s * plan["rows_per_split"] >= n_out)


# plan properties the parity suite wants to see launched (section C of the file's docstring)
PROPERTIES = {
    "one_block": lambda p, n: p["grid_y"] == 1 and n > 64 and empty_splits(p, n) == 0,   # one split per wave row of a single workgroup row
    "grid_8": lambda p, n: p["grid_y"] == 8,
    "grid_16": lambda p, n: p["grid_y"] == 16,
    "grid_odd": lambda p, n: p["grid_y"] > 8 and p["grid_y"] % 8 != 0,
    "empty_tail": lambda p, n: empty_splits(p, n) >= 1,
    "ragged": lambda p, n: p["grid_y"] > 1 and p["rows_per_split"] % 64 != 0 and empty_splits(p, n) == 0,
    "long": lambda p, n: p["rows_per_split"] >= 512 and p["n_split"] > 1 and empty_splits(p, n) == 0,
    "splits_below_16": lambda p, n: 1 < p["n_split"] < 16,      # against the 16 thread rows of wgrad_reduce4_kernel
    "splits_16": lambda p, n: p["n_split"] == 16,
    "splits_above_16": lambda p, n: p["n_split"] > 16,
}
# 5 rows on four wave rows: splits [0, 4), [4, 5) and two empty ones; 3 rows on two wave rows: one empty; one split per workgroup needs
# 16 897 rows on 66 workgroup rows before the rounding of rows_per_split to a multiple of 4 empties the last one
CHOICE_ROWS = (5, 3, 200, 300, 700, 1100, 1300, 2100, 2300, 3100, 3900, 4100, 4700, 6100, 8000, 8300, 9100, 12300, 16200, 16897, 19000)
CHOICE_BLOCKS = (1, 2, 3, 4, 8, 9, 10, 11, 16, 17, 20, 66)   # S2D_WGRAD_WAVES = 4 * kvol * these


def choose_plan(plan_fn, prop, kvol):
    """the first row count of CHOICE_ROWS, then the smallest S2D_WGRAD_WAVES, whose plan has the property; plan_fn(n_out, waves) -> plan.
    -> (n_out, waves, plan) or None"""
    for n_out in CHOICE_ROWS:
        for g in CHOICE_BLOCKS:
            plan = plan_fn(n_out, 4 * kvol * g)
            if PROPERTIES[prop](plan, n_out):
                return n_out, 4 * kvol * g, plan
    return None


# ---- operands, maps, reference -------------------------------------------------------------------------------------------------------------
def exact_operands(n_in, n_out, cin, cout, seed):
    """-> feat fp32 [n_in, cin], dout fp32 [n_out, cout], and the same values as bf16; integers in {-3 .. 3} (CPU tensors)"""
    assert 0 <= n_out < MAX_ROWS, "9 * n_out must stay below 2^24 for fp32 sums of the products to be exact"
    g = torch.Generator().manual_seed(seed)
    feat = torch.randint(-3, 4, (n_in, cin), generator=g).float()
    dout = torch.randint(-3, 4, (n_out, cout), generator=g).float()
    return feat, dout, feat.bfloat16(), dout.bfloat16()


def density_map(kvol, n_in, n_out, p, seed, empty_block=True, spare_zero=False):
    """gather map int32 [kvol, n_out]: each (offset, row) has a neighbour with probability p; empty_block: rows 16..63 have none at any
    offset (as test_s16_gpu._random_map); spare_zero: no pair names input row 0 or output row 0"""
    g = torch.Generator().manual_seed(seed)
    lo = 1 if spare_zero and n_in > 1 else 0
    nbr = torch.randint(lo, max(n_in, lo + 1), (kvol, n_out), dtype=torch.int32, generator=g)
    nbr[torch.rand(kvol, n_out, generator=g) >= p] = -1
    if empty_block and n_out > 64:
        nbr[:, 16:64] = -1
    if spare_zero:
        nbr[:, :1] = -1
    return nbr


def dense_map(kvol, n_in, n_out, seed):
    return density_map(kvol, n_in, n_out, 2.0, seed, empty_block=False)


def empty_map(kvol, n_out):
    return torch.full((kvol, n_out), -1, dtype=torch.int32)


def one_pair_map(kvol, n_in, n_out, seed):
    """one pair in the whole map, away from input row 0 and output row 0 where the sizes allow it"""
    nbr = empty_map(kvol, n_out)
    nbr[seed % kvol, (37 + 41 * seed) % (n_out - 1) + 1 if n_out > 1 else 0] = (5 + 3 * seed) % (n_in - 1) + 1 if n_in > 1 else 0
    return nbr


def last_row_map(kvol, n_in, n_out, seed):
    """every offset has exactly one pair, at the last output row"""
    g = torch.Generator().manual_seed(seed)
    nbr = empty_map(kvol, n_out)
    nbr[:, n_out - 1] = torch.randint(1 if n_in > 1 else 0, n_in, (kvol,), dtype=torch.int32, generator=g)
    return nbr


def window_gap_map(kvol, n_in, n_out, seed):
    """64-row windows alternately full and empty (which ones, shifted per offset)"""
    nbr = dense_map(kvol, n_in, n_out, seed)
    win = torch.arange(n_out) // 64
    for k in range(kvol):
        nbr[k, (win + k) % 2 == 1] = -1
    return nbr


def poisoned_operands(feat, dout, nbr):
    """copies of feat / dout with NaN in the rows the reference never reads: input rows no pair names, gradient rows without a neighbour
    at any offset.  A kernel's clamped gather may load them; its select must keep them out of the sums."""
    valid = nbr >= 0
    used_in = torch.zeros(feat.shape[0], dtype=torch.bool)
    used_in[nbr[valid].long()] = True
    used_out = valid.any(0)
    feat, dout = feat.clone(), dout.clone()
    feat[~used_in] = float("nan")
    dout[~used_out] = float("nan")
    return feat, dout


def exact_reference(feat, dout, nbr):
    """int64 [kvol, cin, cout]: gather(feat, nbr[k])^T @ dout per offset over the pairs of the map, rows outside them never read.
    Evaluated as a float64 matmul (integers below 2^53: exact in any order, and it runs on either device) and converted; the conversion is
    checked to be lossless, and tests/test_spconv_wgrad_checks_cpu.py compares it with the integer matmul."""
    kvol, cin, cout = nbr.shape[0], feat.shape[1], dout.shape[1]
    ref = torch.zeros(kvol, cin, cout, dtype=torch.float64, device=feat.device)
    for k in range(kvol):
        o = torch.nonzero(nbr[k] >= 0).squeeze(1)
        if o.numel():
            ref[k] = feat[nbr[k][o].long()].double().t() @ dout[o].double()
    out = ref.to(torch.int64)
    assert bool((out.double() == ref).all()) and int(out.abs().max()) < (1 << 24)
    return out


def pair_counts(nbr):
    return (nbr >= 0).sum(1)


@functools.lru_cache(maxsize=None)
def exact_case(map_kind, kvol, n_in, n_out, cin, cout, seed, p=0.5, device="cpu"):
    """one problem, built once and never modified: -> dict(feat32, dout32, feat16, dout16 (poisoned), nbr, ref int64), CPU tensors;
    device: where the reference's matmuls run"""
    if map_kind == "density":
        nbr = density_map(kvol, n_in, n_out, p, seed, spare_zero=p < 0.1)
    elif map_kind == "dense":
        nbr = dense_map(kvol, n_in, n_out, seed)
    elif map_kind == "empty":
        nbr = empty_map(kvol, n_out)
    elif map_kind == "one_pair":
        nbr = one_pair_map(kvol, n_in, n_out, seed)
    elif map_kind == "last_row":
        nbr = last_row_map(kvol, n_in, n_out, seed)
    elif map_kind == "window_gaps":
        nbr = window_gap_map(kvol, n_in, n_out, seed)
    else:
        raise KeyError(map_kind)
    feat, dout, _, _ = exact_operands(n_in, n_out, cin, cout, 7919 * seed + cin + cout)
    ref = exact_reference(feat.to(device), dout.to(device), nbr.to(device)).cpu()
    feat, dout = poisoned_operands(feat, dout, nbr)
    return dict(feat32=feat, dout32=dout, feat16=feat.bfloat16(), dout16=dout.bfloat16(), nbr=nbr, ref=ref)


# ---- caller-owned buffers and the launch ---------------------------------------------------------------------------------------------------
WS_ROW = 64   # floats per row of the workspace allocation: 256 bytes, the granule of the workspace query


def assert_guards(buf, what):
    """the guard rows of a test_spconv_plans_gpu.poisoned allocation still hold the NaN fill bit for bit"""
    from test_spconv_plans_gpu import GUARD, _bits
    fill = _bits(torch.full((1,), float("nan"), dtype=buf.dtype, device=buf.device)).item()
    bits = _bits(buf).flatten(1)
    for name, g in (("front", bits[:GUARD]), ("back", bits[-GUARD:])):
        assert bool((g == fill).all()), f"{what}: {name} guard rows overwritten ({int((g != fill).sum())} elements)"


def check_buffers(dbuf, wbuf, n_partial):
    """1. guards of dweight and of the workspace bit-unchanged; 2. every element of dweight finite; 3. the first n_partial floats of the
    workspace (n_split * kvol * cin * cout: every split's partial, an empty trailing split's zeros included) finite"""
    from test_spconv_plans_gpu import GUARD, assert_written
    assert_guards(dbuf, "dweight")
    if wbuf is not None:
        assert_guards(wbuf, "workspace")
    assert_written(dbuf, "dweight")
    if wbuf is not None:
        part = wbuf[GUARD:-GUARD].flatten()[:n_partial]
        assert part.numel() == n_partial, ("workspace shorter than the plan's partials", part.numel(), n_partial)
        bad = ~torch.isfinite(part)
        assert not bool(bad.any()), ("workspace: partial sums left at the NaN fill", int(bad.sum()), bad.nonzero().flatten()[:8].tolist())


def alloc_buffers(ws_bytes, kvol, cin, cout, device):
    """-> (dbuf, dweight [kvol, cin, cout], wbuf | None, workspace of exactly ws_bytes | None), NaN-filled between NaN guard rows"""
    from test_spconv_plans_gpu import poisoned
    dbuf, dw = poisoned(kvol, cin, cout, dtype=torch.float32, device=device)
    if ws_bytes == 0:
        return dbuf, dw, None, None
    assert ws_bytes % (4 * WS_ROW) == 0
    wbuf, ws = poisoned(ws_bytes // (4 * WS_ROW), WS_ROW, dtype=torch.float32, device=device)
    return dbuf, dw, wbuf, ws


def run_entry(entry, feat, dout, nbr, kvol):
    """one C-ABI weight-gradient entry ("f32" s2d_spconv_wgrad_f32, "bf16" s2d_spconv_wgrad_bf16, "s16" s2d_spconv_s16_wgrad) on device
    tensors, called directly (hip_ops.spconv_wgrad pads cin): dweight and the workspace - of exactly s2d_spconv_wgrad_workspace_bytes -
    are caller-owned, NaN-filled and fenced; check_buffers runs on them.  -> (dweight fp32 [kvol, cin, cout], plan)"""
    from sparse2dense_amd import _lib, hip_ops as H
    lib = _lib.load()
    mode = ENTRIES[entry]
    (n_in, cin), (n_out, cout) = feat.shape, dout.shape
    assert feat.dtype == dout.dtype == (torch.bfloat16 if entry == "s16" else torch.float32)
    assert feat.is_contiguous() and dout.is_contiguous() and nbr.is_contiguous() and nbr.dtype == torch.int32 and nbr.shape == (kvol, n_out)
    fn = {"f32": lib.s2d_spconv_wgrad_f32, "bf16": lib.s2d_spconv_wgrad_bf16, "s16": lib.s2d_spconv_s16_wgrad}[entry]
    memset_path = n_out == 0 or n_in == 0
    plan = query_plan(mode, n_out, kvol, cin, cout)
    ws_bytes = 0 if memset_path else int(lib.s2d_spconv_wgrad_workspace_bytes(n_out, kvol, cin, cout))
    n_partial = plan["n_split"] * kvol * cin * cout
    assert memset_path or ws_bytes >= 4 * n_partial
    dbuf, dw, wbuf, ws = alloc_buffers(ws_bytes, kvol, cin, cout, feat.device)
    _lib.check(fn(H._ptr(feat), n_in, H._ptr(dout), H._ptr(nbr), n_out, kvol, cin, cout, H._ptr(dw), H._ptr(ws), ws_bytes, H._stream()),
               "s2d_spconv_wgrad " + entry)
    check_buffers(dbuf, wbuf, n_partial)
    return dw, plan


def assert_exact(dw, ref, what=""):
    """torch.equal against the int64 reference (below 2^24 in magnitude, so its fp32 image is exact); no tolerance"""
    want = ref.to(dw.device).float()
    if not torch.equal(dw, want):
        bad = (dw != want).flatten(1).any(1).nonzero().flatten()
        diff = (dw.double() - want.double()).abs()
        raise AssertionError(("dweight differs from the exact reference", what, "offsets", bad[:8].tolist(), "elements", int((dw != want).sum()),
                              "max |diff|", float(diff[torch.isfinite(diff)].max()) if bool(torch.isfinite(diff).any()) else float("nan")))
