"""Forward parity of the bf16 sparse implicit GEMMs (csrc/spconv_rg.hip, csrc/spconv_s16.hip) at EVERY deal of tiles to waves and
behind every launch plan, not only the ones the benchmark's row counts happen to reach.

What a wave of spconv_rg_kernel does depends on tiles_per_block (1..16 for the production <MI = 2, WAVES = 8> shape): its rg_wave<NT>
instantiation (0, 1 or 2 tiles), which waves are phantoms that only keep the barriers, how the last workgroup is cut.  rg_plan derives the
value from the row count and the CU count; both plan functions read their tuning hook (S2D_RG_PLAN = "mi,waves,tiles_per_block",
S2D_S16_PLAN = "bm,rows_per_block") on every launch, so one process sweeps them with monkeypatch.setenv.

Every launch goes through run_plain / run_sorted below: the output and the statistics rows are caller-owned, NaN-filled and fenced by
NaN guard rows; inputs are finite, so a NaN after the launch is a row nobody wrote and a changed guard is a store out of bounds.
Every case then asserts
  1. guards bit-unchanged, every element of out[0:n_out] and of the statistics rows finite                      (check_launch)
  2. |out - ref| <= 8e-3 * max|ref| on every row, ref = the float64 restatement on the same bf16-rounded operands: the one bf16
     rounding of the output is 2^-8 relative (tests/test_s16_gpu.py); the natural-plan cases, up to ~65 500 rows, use that file's
     device-side fp32 reference at its 1.2e-2
  3. the statistics rows fold to the column sums / sums of squares of the STORED rows (rtol 1e-4, atol 1e-2)
  4. the output is torch.equal to the output of the default plan for the same inputs (sorted kernel against sorted kernel): a row's
     accumulator takes the steps and K chunks in the same order whatever MI, WAVES, tiles_per_block, BM or rows_per_block is - in the
     LDS-staged kernel the column split WN only moves a column to another wave - so a mis-dealt tile cannot hide inside a tolerance.
tests/test_spconv_plan_checks_cpu.py shows on the host that these checks reject the r04 defect (second tile of a wave wrong) and a
skipped tile.
"""
import functools

import pytest
import torch

from test_s16_gpu import _SHAPES, _random_map, _ref_conv, _shaped_map, _subm_rulebook

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 2   # guard rows on each side of a caller-owned buffer


# ---- part 0: poisoned, caller-owned outputs -------------------------------------------------------------------------------------------
def poisoned(rows, *row_shape, dtype, device=DEV):
    """-> (the whole allocation, its rows [GUARD : GUARD + rows] that the launch may write), all of it NaN"""
    buf = torch.full((rows + 2 * GUARD,) + tuple(row_shape), float("nan"), dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + rows]


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def assert_written(buf, what):
    """the guard rows of a `poisoned` allocation still hold the fill bit for bit; everything between them is finite"""
    fill = _bits(torch.full((1,), float("nan"), dtype=buf.dtype, device=buf.device)).item()
    bits = _bits(buf).flatten(1)
    for name, g in (("front", bits[:GUARD]), ("back", bits[-GUARD:])):
        assert bool((g == fill).all()), f"{what}: {name} guard rows overwritten ({int((g != fill).sum())} elements)"
    unwritten = (~torch.isfinite(buf[GUARD:-GUARD].flatten(1))).any(1)
    assert not bool(unwritten.any()), (f"{what}: rows left at the NaN fill", int(unwritten.sum()), unwritten.nonzero().flatten()[:8].tolist())


def check_launch(obuf, pbuf):
    assert_written(obuf, "out")
    if pbuf is not None:
        assert_written(pbuf, "partial")


def _stats_tiles(n_out, kvol, cin, cout):
    from sparse2dense_amd import _lib
    return int(_lib.load().s2d_spconv_s16_stats_tiles(int(n_out), int(kvol), int(cin), int(cout)))


def run_plain(feat, packed, kvol, cin, cout, bias, nbr, n_out, with_stats=False):
    """s2d_spconv_s16_fwd_stats as hip_ops.spconv_s16_run calls it, into poisoned buffers; -> (out bf16 [n_out, cout], partial | None)"""
    from sparse2dense_amd import _lib, hip_ops as H
    lib = _lib.load()
    assert feat.dtype == torch.bfloat16 and feat.shape[1] == cin and feat.is_contiguous() and nbr.is_contiguous() and n_out > 0
    obuf, out = poisoned(n_out, cout, dtype=torch.bfloat16, device=feat.device)
    pbuf = partial = None
    if with_stats:
        pbuf, partial = poisoned(_stats_tiles(n_out, kvol, cin, cout), 2, cout, dtype=torch.float32, device=feat.device)
    _lib.check(lib.s2d_spconv_s16_fwd_stats(H._ptr(feat), feat.shape[0], H._ptr(packed), H._ptr(bias), H._ptr(nbr), int(n_out), kvol, cin, cout,
                                            H._ptr(H.zero_page(feat.device)), H._ptr(out), H._ptr(partial), H._stream()), "s2d_spconv_s16_fwd_stats")
    check_launch(obuf, pbuf)
    return out, partial


def run_sorted(feat, packed, kvol, cin, cout, bias, rb, with_stats=False):
    """s2d_spconv_s16_fwd_sorted as hip_ops.spconv_s16_run_sorted calls it, into poisoned buffers"""
    from sparse2dense_amd import _lib, hip_ops as H
    lib = _lib.load()
    n_out = int(rb.n_out)
    assert feat.dtype == torch.bfloat16 and feat.shape[1] == cin and feat.is_contiguous() and n_out > 0
    perm, pmask, nbr_perm = H.rulebook_sorted_rows(rb)
    obuf, out = poisoned(n_out, cout, dtype=torch.bfloat16, device=feat.device)
    pbuf = partial = None
    if with_stats:
        pbuf, partial = poisoned(_stats_tiles(n_out, kvol, cin, cout), 2, cout, dtype=torch.float32, device=feat.device)
    _lib.check(lib.s2d_spconv_s16_fwd_sorted(H._ptr(feat), feat.shape[0], H._ptr(packed), H._ptr(bias), H._ptr(nbr_perm), H._ptr(perm), H._ptr(pmask),
                                             n_out, kvol, cin, cout, H._ptr(out), H._ptr(partial), H._stream()), "s2d_spconv_s16_fwd_sorted")
    check_launch(obuf, pbuf)
    return out, partial


# ---- what each case asserts about a launch's results ------------------------------------------------------------------------------------
def assert_parity(out, ref, tol=8e-3):
    """every row within tol * max|ref| of the reference (a NaN is a miss)"""
    bad = ~((out.to(ref.dtype) - ref).abs() <= tol * ref.abs().max()).all(1)
    assert int(bad.sum()) == 0, ("rows off the reference", int(bad.sum()), bad.nonzero().flatten()[:8].tolist())


def assert_stats(out, partial):
    part, o64 = partial.double().sum(0), out.double()
    assert torch.allclose(part[0], o64.sum(0), rtol=1e-4, atol=1e-2), "sum rows of the epilogue != column sums of the stored rows"
    assert torch.allclose(part[1], (o64 * o64).sum(0), rtol=1e-4, atol=1e-2), "square-sum rows of the epilogue != those of the stored rows"


def assert_same_bits(out, base):
    if not torch.equal(out, base):
        rows = (out != base).any(1).nonzero().flatten()
        raise AssertionError(("rows differ from the default plan's output", int(rows.numel()), rows[:8].tolist()))


def check_output(out, partial, ref, base=None, tol=8e-3):
    assert_parity(out, ref, tol)
    if partial is not None:
        assert_stats(out, partial)
    if base is not None:
        assert_same_bits(out, base)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
PLAIN_SHAPES = [(64, 128), (128, 64), (128, 128)]   # the register-gather kernel's shapes (64 -> 64 and narrower: the LDS-staged kernel, _LDS_SHAPES)
N_IN = 300


def ceil_div(a, b):
    return -(-a // b)


def rows_for(t):
    """two full workgroups of t tiles and a third that is partly dealt, with a ragged last tile"""
    return 16 * (2 * t + max(1, t // 2)) - 5


@functools.lru_cache(maxsize=None)
def _operands(cin, cout, kvol, n_in=N_IN):
    g = torch.Generator(device=DEV).manual_seed(1000 * cin + 10 * cout + kvol)
    feat = torch.randn(n_in, cin, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(kvol, cin, cout, device=DEV, generator=g) * 0.1
    bias = torch.randn(cout, device=DEV, generator=g)
    return feat, w, bias


@functools.lru_cache(maxsize=None)
def _plain_problem(cin, cout, kvol, n_out, dgrad=False):
    """operands, gather map and float64 reference of one case (shared, never modified).  dgrad: the data-gradient operand - the weight
    stored [K, cout_fwd, cin_fwd], packed transposed with the offsets mirrored"""
    feat, w, bias = _operands(cin, cout, kvol)
    nbr = _random_map(kvol, N_IN, n_out, p_empty=0.5, seed=n_out + kvol)
    if dgrad:
        return feat, w.transpose(1, 2).contiguous(), bias, nbr, _ref_conv(feat, w.flip(0), bias, nbr, n_out)
    return feat, w, bias, nbr, _ref_conv(feat, w, bias, nbr, n_out)


def _run_plain_plan(monkeypatch, var, plan, cin, cout, kvol, n_out, dgrad=False):
    """both launches (without / with the statistics epilogue) of one problem under one plan (None: no override), weights packed under the
    same environment; each checked against the reference; -> the output"""
    from sparse2dense_amd import hip_ops as H
    feat, w, bias, nbr, ref = _plain_problem(cin, cout, kvol, n_out, dgrad)
    if plan is None:
        monkeypatch.delenv(var, raising=False)
    else:
        monkeypatch.setenv(var, plan)
    packed, kv, ci, co = H.spconv_s16_pack(w, n_out, transpose=dgrad, flip=dgrad)
    assert (kv, ci, co) == (kvol, cin, cout)
    out, _ = run_plain(feat, packed, kv, ci, co, bias, nbr, n_out, False)
    out_s, partial = run_plain(feat, packed, kv, ci, co, bias, nbr, n_out, True)
    check_output(out, None, ref)
    check_output(out_s, partial, ref, out)
    return out


def _check_rg_plan(monkeypatch, mi, waves, t, cin, cout, kvol=27, dgrad=False):
    n_out = rows_for(t)
    for v in ("S2D_RG_PLAN", "S2D_S16_PLAN"):
        monkeypatch.delenv(v, raising=False)
    base = _run_plain_plan(monkeypatch, "S2D_RG_PLAN", None, cin, cout, kvol, n_out, dgrad)
    monkeypatch.setenv("S2D_RG_PLAN", f"{mi},{waves},{t}")
    assert _stats_tiles(n_out, kvol, cin, cout) == ceil_div(ceil_div(n_out, 16), t), "the forced plan was not taken"
    out = _run_plain_plan(monkeypatch, "S2D_RG_PLAN", f"{mi},{waves},{t}", cin, cout, kvol, n_out, dgrad)
    assert_same_bits(out, base)


@functools.lru_cache(maxsize=None)
def _sorted_problem(c, n, kind, p_drop):
    g = torch.Generator(device=DEV).manual_seed(77 * c + n)
    feat = torch.randn(n, c, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(27, c, c, device=DEV, generator=g) * 0.1
    bias = torch.randn(c, device=DEV, generator=g)
    nbr = _shaped_map(n, _SORTED_SHAPES[kind], seed=7 * n + c, p_drop=p_drop)
    return feat, w, bias, nbr, _ref_conv(feat, w, bias, nbr, n)


# masks of one, two, four and five kernel offsets (the centre among them): the sorted kernel's step list comes from the masks, not from kvol
_SORTED_SHAPES = dict(_SHAPES, two=[(1 << 13) | (1 << 4)], four=[(1 << 13) | (1 << 2) | (1 << 17) | (1 << 26)],
                      five=[(1 << 13) | (1 << 0) | (1 << 5) | (1 << 20) | (1 << 26)])


def _check_sorted_plan(monkeypatch, t, c, kind, p_drop=0.0):
    from sparse2dense_amd import hip_ops as H
    n = rows_for(t)
    for v in ("S2D_RG_PLAN", "S2D_S16_PLAN"):
        monkeypatch.delenv(v, raising=False)
    feat, w, bias, nbr, ref = _sorted_problem(c, n, kind, p_drop)
    rb = _subm_rulebook(nbr)
    was = H.set_sorted_rows(True)
    try:
        assert H.spconv_s16_sorted_ok(rb, 27, c, c, n)
        outs = {}
        for plan in (None, f"2,8,{t}"):
            if plan is not None:
                monkeypatch.setenv("S2D_RG_PLAN", plan)
                assert _stats_tiles(n, 27, c, c) == ceil_div(ceil_div(n, 16), t), "the forced plan was not taken"
            packed, kv, ci, co = H.spconv_s16_pack(w, n)
            out, _ = run_sorted(feat, packed, kv, ci, co, bias, rb, False)
            out_s, partial = run_sorted(feat, packed, kv, ci, co, bias, rb, True)
            check_output(out, None, ref)
            check_output(out_s, partial, ref, out)
            outs[plan] = out
        assert_same_bits(outs[f"2,8,{t}"], outs[None])
    finally:
        H.set_sorted_rows(was)


# ---- part 1: every tile deal of the production instantiation ---------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", PLAIN_SHAPES)
@pytest.mark.parametrize("t", range(1, 17))
def test_rg_every_tile_deal(t, cin, cout, monkeypatch):
    """<MI = 2, WAVES = 8> with tiles_per_block forced to t: t <= 8 leaves 8 - t phantom waves and one tile on the others, t > 8 gives
    t - 8 waves a second tile; two full workgroups and a third with max(1, t // 2) tiles, the last one ragged"""
    _check_rg_plan(monkeypatch, 2, 8, t, cin, cout)


@pytest.mark.parametrize("cin,cout", PLAIN_SHAPES)
def test_rg_data_gradient_operand_with_two_tiles_per_wave(cin, cout, monkeypatch):
    _check_rg_plan(monkeypatch, 2, 8, 11, cin, cout, dgrad=True)


@pytest.mark.parametrize("c", [128])
@pytest.mark.parametrize("t", range(1, 17))
def test_rg_sorted_every_tile_deal(t, c, monkeypatch):
    _check_sorted_plan(monkeypatch, t, c, "mixed", 0.2)
    _check_sorted_plan(monkeypatch, t, c, "plane")


# ---- part 2: step-count edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", PLAIN_SHAPES)
@pytest.mark.parametrize("kvol", [1, 2, 4, 5])
def test_rg_step_count_edges(kvol, cin, cout, monkeypatch):
    """step counts 1, 2, 4, 5 at 128 input channels; a half-filled single step, 1, 2 and 2 1/2 steps at 64 - padded to even with phantom
    steps; indices are requested four steps ahead and weight slabs two, so at one step the whole prologue is phantom"""
    for t in (1, 11):
        _check_rg_plan(monkeypatch, 2, 8, t, cin, cout, kvol=kvol)


@pytest.mark.parametrize("c", [128])
@pytest.mark.parametrize("kind", ["centre", "two", "four", "five"])
def test_rg_sorted_step_count_edges(kind, c, monkeypatch):
    """the sorted kernel's kvol is 27: short step lists come from the masks (every row the same one, two, four or five offsets)"""
    for t in (1, 11):
        _check_sorted_plan(monkeypatch, t, c, kind)


# ---- part 3: natural plans on the device the suite runs on ------------------------------------------------------------------------------
def _natural_tiles_per_block(tiles, cus):
    rounds = max(1, ceil_div(tiles, 16 * cus))
    return min(16, ceil_div(tiles, cus * rounds))


@pytest.mark.parametrize("t,cin,cout", [(2, 128, 128), (5, 128, 128), (8, 128, 128), (9, 128, 128), (16, 128, 128), (16, 64, 128), (None, 128, 128)],
                         ids=lambda v: "two_rounds" if v is None else str(v))
def test_rg_natural_plans(t, cin, cout, monkeypatch):
    """no override: row counts at which rg_plan itself deals t tiles per workgroup on THIS device's CU count (t None: one tile more than a
    single round of 16-tile workgroups holds); fp32 reference on the device, every row"""
    for v in ("S2D_RG_PLAN", "S2D_S16_PLAN"):
        monkeypatch.delenv(v, raising=False)
    from sparse2dense_amd import hip_ops as H
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = 16 * cus + 1 if t is None else cus * (t - 1) + 1
    n_out, n_in, kvol = 16 * tiles - 3, 3000, 3
    tpb = _natural_tiles_per_block(tiles, cus)
    assert tpb == (t if t is not None else ceil_div(tiles, 2 * cus))
    assert _stats_tiles(n_out, kvol, cin, cout) == ceil_div(tiles, tpb), "rg_plan chose another tiles_per_block"
    g = torch.Generator(device=DEV).manual_seed(tiles)
    feat = torch.randn(n_in, cin, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(kvol, cin, cout, device=DEV, generator=g) * 0.1
    bias = torch.randn(cout, device=DEV, generator=g)
    nbr = _random_map(kvol, n_in, n_out, p_empty=0.5, seed=tiles)
    ref = torch.zeros(n_out, cout, device=DEV, dtype=torch.float32) + bias
    fr, wr = feat.float(), w.to(torch.bfloat16).float()
    for k in range(kvol):
        o = torch.nonzero(nbr[k] >= 0).squeeze(1)
        ref[o] += fr[nbr[k][o].long()] @ wr[k]
    packed, kv, ci, co = H.spconv_s16_pack(w, n_out)
    out, _ = run_plain(feat, packed, kv, ci, co, bias, nbr, n_out, False)
    out_s, partial = run_plain(feat, packed, kv, ci, co, bias, nbr, n_out, True)
    check_output(out, None, ref, tol=1.2e-2)
    check_output(out_s, partial, ref, out, tol=1.2e-2)


# ---- part 4: the instantiations behind the tuning hooks ---------------------------------------------------------------------------------
_HOOK_PLANS = [(mi, waves, cin, cout) for mi, waves in [(1, 8), (1, 4), (2, 4), (3, 4), (4, 4)] for cin, cout in PLAIN_SHAPES] + \
              [(3, 8, 128, 64), (4, 8, 128, 64)]   # (3+, 8) needs more registers than a wave has at 128 output channels: the parser refuses it


@pytest.mark.parametrize("mi,waves,cin,cout", _HOOK_PLANS)
def test_rg_tuning_hook_instantiation(mi, waves, cin, cout, monkeypatch):
    """spconv_rg_kernel<cin, cout, mi, waves>, reachable only through S2D_RG_PLAN (tools/spconv_kernel_bench.py A/B runs): one tile per
    workgroup, a deal that gives half of the waves one tile more than the others, and the full mi * waves tiles"""
    for t in (1, mi * waves // 2 + 1, mi * waves):
        _check_rg_plan(monkeypatch, mi, waves, t, cin, cout)


@pytest.mark.parametrize("plan,cin,cout", [("3,8,5", 128, 128), ("4,8,5", 64, 128), ("5,8,3", 128, 64), ("2,6,3", 128, 64), ("0,8,3", 128, 128)])
def test_rg_rejected_plan_leaves_the_default_in_force(plan, cin, cout, monkeypatch):
    """a plan the parser refuses is ignored as a whole: the grid is the default plan's (the forced tiles_per_block would give another one)
    and so are the bits"""
    n_out, kvol = rows_for(5), 27
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = ceil_div(n_out, 16)
    default_grid = ceil_div(tiles, _natural_tiles_per_block(tiles, cus))
    forced = int(plan.split(",")[2])
    assert default_grid != ceil_div(tiles, forced)
    monkeypatch.delenv("S2D_RG_PLAN", raising=False)
    assert _stats_tiles(n_out, kvol, cin, cout) == default_grid
    base = _run_plain_plan(monkeypatch, "S2D_RG_PLAN", None, cin, cout, kvol, n_out)
    monkeypatch.setenv("S2D_RG_PLAN", plan)
    assert _stats_tiles(n_out, kvol, cin, cout) == default_grid
    assert_same_bits(_run_plain_plan(monkeypatch, "S2D_RG_PLAN", plan, cin, cout, kvol, n_out), base)


def test_rg_plan_with_tiles_per_block_out_of_range_keeps_the_natural_deal(monkeypatch):
    """mi and waves are taken, a tiles_per_block above mi * waves is not: rg_plan derives it as usual"""
    n_out, kvol, cin, cout = rows_for(5), 27, 128, 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = ceil_div(n_out, 16)
    monkeypatch.delenv("S2D_RG_PLAN", raising=False)
    base = _run_plain_plan(monkeypatch, "S2D_RG_PLAN", None, cin, cout, kvol, n_out)
    monkeypatch.setenv("S2D_RG_PLAN", "1,4,5")
    assert _stats_tiles(n_out, kvol, cin, cout) == ceil_div(tiles, min(4, ceil_div(tiles, cus * max(1, ceil_div(tiles, 4 * cus)))))
    assert_same_bits(_run_plain_plan(monkeypatch, "S2D_RG_PLAN", "1,4,5", cin, cout, kvol, n_out), base)


_LDS_SHAPES = [(16, 16), (32, 64), (64, 64), (16, 128), (64, 32)]   # served by the LDS-staged kernel by default


@pytest.mark.parametrize("cin,cout,bm", [(ci, co, bm) for ci, co in _LDS_SHAPES for bm in (64, 128, 256) if not (bm == 256 and co == 128)])
def test_s16_tuning_hook_instantiation(cin, cout, bm, monkeypatch):
    """spconv_fwd_s16_kernel<cin, cout, bm> with rows_per_block at 16, between half and full, and at the template height (the tiles past
    rows_per_block stay unmarked); the weight image is packed under the same plan - its column split depends on bm.  Bit-equal to the
    default plan's output with its own image: per output element the K-steps and the two 32-deep halves of each come in the same order
    whatever bm is; the column split decides only which wave owns a column"""
    from sparse2dense_amd import hip_ops as H
    for v in ("S2D_RG_PLAN", "S2D_S16_PLAN"):
        monkeypatch.delenv(v, raising=False)
    was = H.set_sorted_rows(False)   # (the product's default)
    try:
        for rpb in (16, bm // 2 + 16, bm):
            n_out = 3 * rpb - 5
            base = _run_plain_plan(monkeypatch, "S2D_S16_PLAN", None, cin, cout, 27, n_out)
            monkeypatch.setenv("S2D_S16_PLAN", f"{bm},{rpb}")
            assert _stats_tiles(n_out, 27, cin, cout) == 3, "the forced plan was not taken"
            try:
                assert_same_bits(_run_plain_plan(monkeypatch, "S2D_S16_PLAN", f"{bm},{rpb}", cin, cout, 27, n_out), base)
            except AssertionError as e:
                raise AssertionError((f"rows_per_block {rpb}",) + e.args) from e
    finally:
        H.set_sorted_rows(was)
