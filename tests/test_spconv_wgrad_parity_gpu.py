"""Exact parity of the sparse weight gradient (csrc/spconv.hip) for every kernel behind its three C-ABI entries and every kind of row-split
plan, not only the ones the default picks at a few row counts.

  entry                  kernels
  s2d_spconv_wgrad_f32   spconv_wgrad_mfma<CIN, COUT>                                                                   (kernel id 0)
  s2d_spconv_wgrad_bf16  spconv_wgrad_bf16<CIN, COUT, float>                                                            (1)
  s2d_spconv_s16_wgrad   spconv_wgrad_s16_tr (2; cin <= 64, or S2D_WGRAD_TR=1), spconv_wgrad_s16_coop128 (3; 128 -> 64 / 128),
                         spconv_wgrad_bf16<.., __bf16> (1; 128 -> 16 / 32, S2D_WGRAD_TR=0, S2D_WGRAD_COOP=0)
  the first two          spconv_wgrad_valu (4) when a channel count is not 16 / 32 / 64 / 128
  all                    wgrad_reduce4_kernel, or wgrad_reduce_kernel when kvol * cin * cout is not a multiple of 4

Operands are small integers (tests/spconv_wgrad_ref.py): fp32 accumulation is exact in any order, so every case asserts
torch.equal(dW, int64 reference) - no tolerance; one dropped, doubled, mis-paired or (0, 0)-replaced pair fails it.  Rows the reference
never reads hold NaN, so a clamped gather that is not zeroed by its select fails too.  Every launch goes through R.run_entry: dweight and
a workspace of exactly s2d_spconv_wgrad_workspace_bytes are caller-owned, NaN-filled and fenced; guards unchanged, dweight finite, every
split's partial (an empty trailing split's zeros included) finite.  Every launch runs twice and the second result equals the first.

The hooks S2D_WGRAD_TR / _COOP / _WAVES are read on every launch; a case that forces one first asserts through s2d_spconv_wgrad_plan
that the intended kernel and plan property were taken (a case whose precondition fails is a test bug, it fails).  Two seeds per case.
Sections:
  A  all 16 channel shapes x the three entries, default plan                   D  pair-ring / chunk / window edges, empty maps, n = 0
  B  every kernel choice behind the hooks                                      E  the VALU kernel and both reductions
  C  split-plan edges per kernel family: one workgroup row, grid_y 8 and 16 (wgrad_block's remap, also at kvol 8 and 1), grid_y above 8
     and no multiple of 8, empty trailing splits, rows_per_split off the 64-row window, rows_per_split >= 512 on a dense map
  F  rounding of the fp32 -> bf16 entry (the one case with a tolerance)        G  the host restatement of the plan equals the library's
tests/test_spconv_wgrad_checks_cpu.py shows on the host that these checks reject the seeded defects.
"""
import pytest
import torch

import spconv_wgrad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEDS = (1, 2)
N_IN, N_OUT = 200, 333


def _hooks(monkeypatch, **hooks):
    """S2D_WGRAD_<name> for each keyword (tr, coop, waves); the others unset"""
    for h in R.HOOKS:
        monkeypatch.delenv(h, raising=False)
    for name, v in hooks.items():
        monkeypatch.setenv("S2D_WGRAD_" + name.upper(), str(v))


def _case(*a):
    return R.exact_case(*a, device=DEV)   # (the float64 matmuls of the reference run on the device)


def _launch_exact(entry, case, kvol, kernel=None, prop=None):
    """the case's operands through `entry`, twice; asserts the kernel id / plan property first; -> the plan"""
    sfx = "16" if entry == "s16" else "32"
    feat, dout, nbr = case["feat" + sfx].to(DEV), case["dout" + sfx].to(DEV), case["nbr"].to(DEV)
    plan = R.query_plan(R.ENTRIES[entry], dout.shape[0], kvol, feat.shape[1], dout.shape[1])
    if kernel is not None:
        assert plan["kernel"] == kernel, ("the intended kernel was not taken", R.KERNELS[kernel], plan)
    if prop is not None:
        assert R.PROPERTIES[prop](plan, dout.shape[0]), ("the intended plan property was not taken", prop, plan)
    dw, ran = R.run_entry(entry, feat, dout, nbr, kvol)
    assert ran == plan
    R.assert_exact(dw, case["ref"], (entry, plan))
    again, _ = R.run_entry(entry, feat, dout, nbr, kvol)
    assert torch.equal(again, dw), "the second launch on the same operands differs from the first"
    return plan


def _default_kernel(entry, cin, cout):
    if entry != "s16":
        return R.ENTRIES[entry]
    return 2 if cin <= 64 else 3 if cout >= 64 else 1


# ---- A: every shape of every entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", list(R.ENTRIES))
@pytest.mark.parametrize("cin,cout", R.SHAPES16)
def test_every_shape_of_every_entry(cin, cout, entry, monkeypatch):
    """333 rows (ragged last window), density 0.5, rows 16..63 without a neighbour, 27 offsets"""
    _hooks(monkeypatch)
    for seed in SEEDS:
        _launch_exact(entry, _case("density", 27, N_IN, N_OUT, cin, cout, seed), 27, kernel=_default_kernel(entry, cin, cout))


# ---- B: every kernel choice --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", R.SHAPES16)
def test_register_assembled_kernel_on_bf16_storage(cin, cout, monkeypatch):
    """S2D_WGRAD_TR=0 (and S2D_WGRAD_COOP=0 where the cooperative kernel would step in): spconv_wgrad_bf16<.., __bf16> at all 16 shapes"""
    _hooks(monkeypatch, tr=0, coop=0)
    for seed in SEEDS:
        _launch_exact("s16", _case("density", 27, N_IN, N_OUT, cin, cout, seed), 27, kernel=1)


@pytest.mark.parametrize("cout", R.MFMA_CHANNELS)
def test_transpose_read_kernel_at_128_input_channels(cout, monkeypatch):
    """S2D_WGRAD_TR=1: spconv_wgrad_s16_tr<128, cout> (NBMAX = 2), which the default never launches"""
    _hooks(monkeypatch, tr=1)
    for seed in SEEDS:
        _launch_exact("s16", _case("density", 27, N_IN, N_OUT, 128, cout, seed), 27, kernel=2)


@pytest.mark.parametrize("cout", [64, 128])
def test_cooperative_kernel_switched_off(cout, monkeypatch):
    """S2D_WGRAD_COOP=0 alone: 128 -> 64 / 128 falls to the register-assembled kernel; S2D_WGRAD_TR=0 alone keeps the cooperative one"""
    _hooks(monkeypatch, coop=0)
    for seed in SEEDS:
        _launch_exact("s16", _case("density", 27, N_IN, N_OUT, 128, cout, seed), 27, kernel=1)
    _hooks(monkeypatch, tr=0)
    _launch_exact("s16", _case("density", 27, N_IN, N_OUT, 128, cout, 1), 27, kernel=3)


# ---- C: split-plan edges ------------------------------------------------------------------------------------------------------------------
# family -> entry, hooks, kernel id, narrow shape, wide shape, the shape nearest to the wide one with two wave rows per workgroup
C_FAMILIES = {
    "mfma_f32": ("f32", {}, 0, (16, 16), (128, 128), (128, 64)),
    "bf16_reg": ("bf16", {}, 1, (16, 16), (128, 128), (128, 64)),
    "bf16_reg_s16": ("s16", dict(tr=0, coop=0), 1, (16, 16), (128, 128), (128, 64)),
    "tr": ("s16", dict(tr=1), 2, (16, 16), (128, 128), (128, 64)),
    "coop": ("s16", {}, 3, (128, 64), (128, 128), None),
}
C_PROPS = ("one_block", "grid_8", "grid_16", "grid_odd", "empty_tail", "ragged", "long")


def _c_cases():
    out = []
    for fam, (_, _, _, narrow, wide, wide2) in C_FAMILIES.items():
        for which, shape in (("narrow", narrow), ("wide", wide)):
            for prop in C_PROPS:
                if fam == "tr" and prop == "grid_odd":
                    continue   # wgrad_plan rounds the transpose-read kernel's grid_y down to a multiple of 8 once it reaches 8 (G asserts it)
                kvols = (27, 8, 1) if prop in ("grid_8", "grid_16") else (27,)
                if fam == "tr" and prop == "empty_tail" and which == "wide":
                    shape_ = wide2   # one split per workgroup and grid_y a multiple of 8: no empty split below 20 000 rows
                else:
                    shape_ = shape
                out += [(fam, shape_, prop, kvol) for kvol in kvols]
    return out


@pytest.mark.parametrize("fam,shape,prop,kvol", _c_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_split_plan_edges(fam, shape, prop, kvol, monkeypatch):
    """row count and S2D_WGRAD_WAVES chosen with the plan query (R.choose_plan) so that the launch has the property; dense map for
    rows_per_split >= 512 (64 pairs per window: the ring of 256 slots wraps, chunks cross windows), density 0.5 otherwise"""
    entry, hooks, kernel, _, _, _ = C_FAMILIES[fam]
    cin, cout = shape

    def plan_fn(n_out, waves):
        _hooks(monkeypatch, waves=waves, **hooks)
        return R.query_plan(R.ENTRIES[entry], n_out, kvol, cin, cout)
    chosen = R.choose_plan(plan_fn, prop, kvol)
    assert chosen is not None, "no row count / S2D_WGRAD_WAVES of the candidate lists gives this plan"
    n_out, waves, plan = chosen
    assert n_out <= 20000
    _hooks(monkeypatch, waves=waves, **hooks)
    for seed in SEEDS:
        case = _case("dense" if prop == "long" else "density", kvol, N_IN, n_out, cin, cout, seed)
        assert _launch_exact(entry, case, kvol, kernel=kernel, prop=prop) == plan
    if prop == "empty_tail" and plan["wrow"] == 4:
        assert n_out == 5 and R.empty_splits(plan, n_out) == 2


# ---- D: ring, chunk and window edges -----------------------------------------------------------------------------------------------------
D_KERNELS = [("f32", 16, 16, 0), ("bf16", 32, 64, 1), ("s16", 16, 16, 2), ("s16", 64, 128, 2), ("s16", 128, 64, 3), ("s16", 128, 128, 3),
             ("s16", 128, 32, 1)]
D_MAPS = [("dense", n, 40, 1.0) for n in (1, 31, 32, 33, 63, 64, 65, 127, 129)] + [
    ("density", 700, N_IN, 0.55),    # ~36 pairs per window: a 32-pair chunk and a 4-pair rest that joins the next window's pairs
    ("density", 700, N_IN, 0.03),    # ~2 pairs per window; no pair names input row 0 or output row 0 (both NaN)
    ("one_pair", 700, N_IN, 0.0), ("last_row", 700, N_IN, 0.0), ("window_gaps", 700, N_IN, 1.0),
    ("density", 333, 1, 0.5),        # n_in = 1: every pair names row 0
    ("empty", 700, N_IN, 0.0)]


@pytest.mark.parametrize("entry,cin,cout,kernel", D_KERNELS)
@pytest.mark.parametrize("kind,n_out,n_in,p", D_MAPS)
def test_ring_and_chunk_edges(kind, n_out, n_in, p, entry, cin, cout, kernel, monkeypatch):
    _hooks(monkeypatch)
    kvol = 3
    for seed in SEEDS:
        case = _case(kind, kvol, n_in, n_out, cin, cout, seed, p)
        if kind in ("empty", "one_pair", "last_row") or p == 0.03:
            assert bool(torch.isnan(case["feat32"][0]).all()) and bool(torch.isnan(case["dout32"][0]).all())   # the empty ring's clamp target
        if kind == "empty":
            assert int(case["ref"].abs().max()) == 0
        _launch_exact(entry, case, kvol, kernel=kernel)


@pytest.mark.parametrize("entry", list(R.ENTRIES))
@pytest.mark.parametrize("n_in,n_out", [(0, 70), (40, 0), (0, 0)])
def test_no_rows_is_a_memset(n_in, n_out, entry, monkeypatch):
    """n_out = 0 or n_in = 0: dweight exactly zero, no workspace (none is passed)"""
    _hooks(monkeypatch)
    case = _case("empty", 27, n_in, n_out, 16, 32, 1)
    assert int(case["ref"].abs().max()) == 0
    _launch_exact(entry, case, 27)


# ---- E: the VALU kernel and both reductions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["f32", "bf16"])
@pytest.mark.parametrize("prop", ["one_block", "splits_below_16", "splits_16", "splits_above_16"])
@pytest.mark.parametrize("cin,cout,kvol", R.VALU_SHAPES)
def test_valu_kernel_and_both_reductions(cin, cout, kvol, prop, entry, monkeypatch):
    """channel counts off the matrix path: spconv_wgrad_valu, then wgrad_reduce4_kernel ((5, 4, 1): 5 float4 columns, less than one block
    of 16) or wgrad_reduce_kernel ((5, 3, 27) and (3, 3, 3): kvol * cin * cout no multiple of 4); split counts around the 16 thread rows
    of the float4 reduction"""
    def plan_fn(n_out, waves):
        _hooks(monkeypatch, waves=waves)
        return R.query_plan(R.ENTRIES[entry], n_out, kvol, cin, cout)
    chosen = R.choose_plan(plan_fn, prop, kvol)
    assert chosen is not None
    n_out, waves, plan = chosen
    _hooks(monkeypatch, waves=waves)
    for seed in SEEDS:
        assert _launch_exact(entry, _case("density", kvol, N_IN, n_out, cin, cout, seed), kvol, kernel=4, prop=prop) == plan


@pytest.mark.parametrize("cin,cout,kvol", R.VALU_SHAPES)
def test_bf16_storage_entry_refuses_other_channel_counts(cin, cout, kvol):
    from sparse2dense_amd import _lib, hip_ops as H
    lib = _lib.load()
    case = _case("density", kvol, N_IN, N_OUT, cin, cout, 1)
    feat, dout, nbr = case["feat16"].to(DEV), case["dout16"].to(DEV), case["nbr"].to(DEV)
    ws_bytes = int(lib.s2d_spconv_wgrad_workspace_bytes(N_OUT, kvol, cin, cout))
    dbuf, dw, wbuf, ws = R.alloc_buffers(ws_bytes, kvol, cin, cout, DEV)
    rc = lib.s2d_spconv_s16_wgrad(H._ptr(feat), N_IN, H._ptr(dout), H._ptr(nbr), N_OUT, kvol, cin, cout, H._ptr(dw), H._ptr(ws), ws_bytes, H._stream())
    assert rc == -2 and "unsupported channels" in _lib.last_error()   # S2D_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(dbuf).all()) and bool(torch.isnan(wbuf).all()), "a refused call wrote something"


# ---- F: rounding of the fp32 -> bf16 entry --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", [(16, 16), (128, 128)])
def test_fp32_storage_entry_rounds_to_nearest_bf16(cin, cout, monkeypatch, capsys):
    """Strictly positive operands |randn| + 0.5: a truncating (or otherwise biased) conversion moves every product the same way - about
    2^-8 relative, against a bound near 2^-14.  Reference: float64 on the operands rounded by torch's .bfloat16().  Per element
    |dW - ref| <= (P_k + n_split) * 2^-23 * sum |a||b|: the summation bound for P_k products (exact in fp32: 8 x 8 significant bits) and
    the n_split partials, unit roundoff 2^-23 - twice fp32's, so a truncating accumulate passes.
    Largest error / bound measured on MI355X: 16 -> 16 0.0031, 128 -> 128 0.0028 (profiles/spconv_wgrad_parity.txt)."""
    _hooks(monkeypatch)
    kvol, n_in, n_out = 27, N_IN, 700
    g = torch.Generator().manual_seed(cin + cout)
    feat = (torch.randn(n_in, cin, generator=g).abs() + 0.5).to(DEV)
    dout = (torch.randn(n_out, cout, generator=g).abs() + 0.5).to(DEV)
    nbr = R.density_map(kvol, n_in, n_out, 0.5, 3).to(DEV)
    fr, dr = feat.bfloat16().double(), dout.bfloat16().double()
    ref = torch.zeros(kvol, cin, cout, dtype=torch.float64, device=DEV)
    for k in range(kvol):
        o = torch.nonzero(nbr[k] >= 0).squeeze(1)
        ref[k] = fr[nbr[k][o].long()].t() @ dr[o]   # all operands positive: this is sum |a||b| as well
    dw, plan = R.run_entry("bf16", feat, dout, nbr, kvol)
    assert plan["kernel"] == 1
    bound = (R.pair_counts(nbr).double() + plan["n_split"]).view(-1, 1, 1) * 2.0 ** -23 * ref
    ratio = ((dw.double() - ref).abs() / bound).max().item()
    with capsys.disabled():
        print(f"\nspconv_wgrad_bf16 {cin}->{cout}: max error / bound = {ratio:.4f} (n_split {plan['n_split']}, pairs per offset ~{int(R.pair_counts(nbr).float().mean())})")
    assert ratio <= 1.0, ratio


# ---- G: the host restatement of the plan is the library's -------------------------------------------------------------------------------
HOOK_SETTINGS = [{}, dict(tr=0), dict(tr=1), dict(coop=0), dict(waves=216), dict(waves=5000), dict(waves=7)]


def test_mirror_plan_equals_the_library(monkeypatch):
    from sparse2dense_amd import _lib
    lib = _lib.load()
    shapes = R.SHAPES16 + [(ci, co) for ci, co, _ in R.VALU_SHAPES]
    seen = set()
    for hooks in HOOK_SETTINGS:
        _hooks(monkeypatch, **hooks)
        for cin, cout in shapes:
            for kvol in R.GRID_KVOL:
                for n_out in R.GRID_N_OUT + R.CHOICE_ROWS:
                    plans = [R.query_plan(mode, n_out, kvol, cin, cout) for mode in (0, 1, 2)]
                    for mode in (0, 1, 2):
                        assert plans[mode] == R.mirror_plan(mode, n_out, kvol, cin, cout, **hooks), (mode, n_out, kvol, cin, cout, hooks)
                        seen.add(plans[mode]["kernel"])
                        if plans[mode]["kernel"] == 2 and plans[mode]["grid_y"] >= 8:
                            assert plans[mode]["grid_y"] % 8 == 0
                    size = kvol * cin * cout
                    want = R.ceil_div(max(plans[0]["n_split"], plans[2]["n_split"]) * size * 4, 256) * 256
                    assert int(lib.s2d_spconv_wgrad_workspace_bytes(n_out, kvol, cin, cout)) == want, (n_out, kvol, cin, cout, hooks)
    assert seen == {0, 1, 2, 3, 4}


def test_default_plans_at_the_benchmark_row_counts(monkeypatch):
    """no hook set: (kernel, n_split, rows_per_split, grid_y, wrow) of the three entries as before the hooks were read per launch"""
    _hooks(monkeypatch)
    want = {(128, 128, 47890): [(0, 18, 2664, 18, 1), (1, 18, 2664, 18, 1), (3, 18, 2664, 18, 1)],
            (64, 64, 126079): [(0, 36, 3504, 18, 2), (1, 36, 3504, 18, 2), (2, 64, 1972, 16, 4)],
            (64, 128, 47890): [(0, 18, 2664, 18, 1), (1, 18, 2664, 18, 1), (2, 32, 1500, 16, 2)],
            (32, 32, 265026): [(0, 72, 3684, 18, 4), (1, 72, 3684, 18, 4), (2, 128, 2072, 32, 4)],
            (16, 16, 288892): [(0, 72, 4016, 18, 4), (1, 72, 4016, 18, 4), (2, 128, 2260, 32, 4)]}
    assert set(want) == set(R.BENCH_CASES)
    for (cin, cout, n_out), plans in want.items():
        assert [tuple(R.query_plan(mode, n_out, 27, cin, cout).values()) for mode in (0, 1, 2)] == plans, (cin, cout, n_out)
