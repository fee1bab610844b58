"""The checks of tests/convt3d_ref.py reject the defects they are there for (host only, no GPU).

Each defect is made by altering a correct float64 reference result, then fed to the same Report methods that
tests/test_convt3d_variants_gpu.py feeds the kernels' results to; the unaltered result passes the same check.  The last tests restate the
branch each shape of the GPU file is there to reach, from the host model of the launchers (which the GPU file ties to the library)."""
import pytest
import torch

import convt3d_ref as R
import ws_guard

CIN, COUT, SHP = 16, 3, (1, 2, 5, 8)   # rows of 8 cells: every x neighbour of the first and last cell is padding


@pytest.fixture(scope="module")
def small():
    t = R.make_inputs(CIN, COUT, SHP)
    xn = R.normalised(t["x"], t["scale"], t["shift"])
    y, din, dw = R.reference(R.bf16r(xn), t["w"], t["bias"], t["dout"])
    return dict(t, xn=xn, y=y, din=din, dw=dw)


def _passes(fn, *a):
    rep = R.Report()
    assert fn(rep, *a)
    rep.assert_all("correct")


def _rejects(fn, *a):
    rep = R.Report()
    assert not fn(rep, *a)
    with pytest.raises(AssertionError, match="checks failed"):
        rep.assert_all("defect")


def test_correct_results_pass(small):
    _passes(R.Report.f32, "y", small["y"].float(), small["y"])
    _passes(R.Report.bf16, "y16", small["y"].to(torch.bfloat16), small["y"])
    _passes(R.Report.f32, "dW", small["dw"].float(), small["dw"])
    _passes(R.Report.same, "y16 == bf16(y32)", small["y"].float().to(torch.bfloat16), small["y"].to(torch.bfloat16))


def test_normalised_padding_cells_are_rejected(small):
    """a normalise-on-load kernel that applies relu(x * scale + shift) to the zero padding: every border output gains relu(shift) taps"""
    zero = torch.zeros(CIN)
    same = R.reference_with_border(R.bf16r(small["xn"]), zero, small["w"], small["bias"])
    assert (same - small["y"]).abs().max() <= 1e-12 * small["y"].abs().max()       # the construction itself: a zero border is the reference
    border = R.bf16r(torch.relu(small["shift"]))
    assert int((border > 0).sum()) >= CIN // 2
    bad = R.reference_with_border(R.bf16r(small["xn"]), border, small["w"], small["bias"])
    _rejects(R.Report.f32, "y", bad.float(), small["y"])
    _rejects(R.Report.bf16, "y16", bad.to(torch.bfloat16), small["y"])


def test_dropped_last_row_block_of_a_weight_gradient_is_rejected(small):
    x = R.bf16r(small["xn"]).clone()
    x[-1, :, -1, -1, :] = 0   # the last (n, z, y) input row contributes nothing: its block never ran / its slab was not summed
    _, _, bad = R.reference(x, small["w"], small["bias"], small["dout"])
    _rejects(R.Report.f32, "dW", bad.float(), small["dw"])


def test_one_swapped_kx_tap_is_rejected(small):
    bad = small["dw"].clone()
    bad[..., 1], bad[..., 3] = small["dw"][..., 3], small["dw"][..., 1]
    _rejects(R.Report.f32, "dW", bad.float(), small["dw"])
    w = small["w"].clone()
    w[..., 0], w[..., 2] = small["w"][..., 2], small["w"][..., 0]
    ybad, dinbad, _ = R.reference(R.bf16r(small["xn"]), w, small["bias"], small["dout"])
    _rejects(R.Report.f32, "y", ybad.float(), small["y"])
    _rejects(R.Report.bf16, "y16", ybad.to(torch.bfloat16), small["y"])
    _rejects(R.Report.f32, "din", dinbad.float(), small["din"])


def test_truncated_bf16_output_is_rejected(small):
    y32 = small["y"].float()
    trunc = (y32.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)   # exact: the low 16 bits are gone
    assert not torch.equal(trunc, y32.to(torch.bfloat16))
    _rejects(R.Report.bf16, "y16", trunc, small["y"])
    _rejects(R.Report.same, "y16 == bf16(y32)", trunc, y32.to(torch.bfloat16))


def test_unwritten_cells_are_rejected(small):
    bad = small["y"].float()
    bad[0, 1, 2, 3, 4] = float("nan")
    _rejects(R.Report.f32, "y", bad, small["y"])
    _rejects(R.Report.bf16, "y16", bad.to(torch.bfloat16), small["y"])
    _rejects(R.Report.same, "identity between two equally unwritten results", bad, bad.clone())


@pytest.mark.parametrize("tiles", [1, 6, 40])
def test_missing_statistics_row_is_rejected(small, tiles):
    stored = small["y"].to(torch.bfloat16)
    good = R.host_partials(stored.float(), tiles)
    _passes(R.Report.stats, "stats", good, stored, tiles)
    for fill in (0.0, float("nan")):   # a block that wrote zeros / a block that never wrote its row (the NaN prefill)
        bad = good.clone()
        bad[tiles // 2] = fill
        _rejects(R.Report.stats, "stats", bad, stored, tiles)
    _rejects(R.Report.stats, "stats", good[:-1] if tiles > 1 else good[:0], stored, tiles)   # a list one row short
    # the statistics are those of the STORED (rounded) values: the sums over the unrounded output are outside the bar
    unrounded = R.host_partials(small["y"].float() * (1 + 2.0 ** -9), tiles)
    _rejects(R.Report.stats, "stats", unrounded, stored, tiles)


@pytest.mark.parametrize("poison", ws_guard.POISONS)
def test_a_write_into_a_guard_is_rejected(poison):
    for offset in (-1, 0, 4095):   # the byte in front of the buffer, the first and a late byte of the back guard
        log = ws_guard.GuardLog(poison)
        buf = log.alloc("convt3d", 1024, "cpu")
        buf.zero_()   # the buffer itself may be written
        _passes(R.Report.guards, "guards", log)
        _, n, base, start, _ = log._allocs[-1]
        base[start + (offset if offset < 0 else n + offset)] = 0
        _rejects(R.Report.guards, "guards", log)


def test_a_touched_output_of_a_refused_call_is_rejected():
    buf = torch.full((64,), 0xFF, dtype=torch.uint8)
    _passes(R.Report.untouched, "outputs untouched", [buf.view(torch.float32), buf.view(torch.bfloat16)], 0xFF)
    buf[17] = 0
    _rejects(R.Report.untouched, "outputs untouched", [buf.view(torch.float32)], 0xFF)
    _rejects(R.Report.rc, "refuses", R.S2D_OK, R.S2D_ERR_UNSUPPORTED)


def test_a_report_travels_as_json():
    rep = R.Report()
    rep.rc("rc", 0, 0)
    rep.rc("refuses", 0, -2)
    back = R.Report.from_json(rep.to_json())
    assert back.items == rep.items and len(back.failures()) == 1
    with pytest.raises(AssertionError, match="nothing was checked"):
        R.Report().assert_all("empty")


# ---- the branch each shape is there for, from the host model of the launchers ---------------------------------------------------------
def _plan(key):
    cin, cout, shp = R.SHAPE[key]
    return R.wgrad_plan(cin, cout, shp)


def _chunks(rows, yc):
    return [min(yc, rows - r) for r in range(0, rows, yc)]


def test_shapes_reach_the_weight_gradient_branches():
    assert _plan("s03_co3")["kind"] == "narrow" and _plan("s03_co3")["rows_per_block"] == 1
    p = _plan("s05")
    assert (p["kind"], p["blocks"], p["rows_per_block"], p["empty"], p["last_rows"]) == ("narrow", 1024, 2, 511, 1)
    p = _plan("s06")
    assert (p["kind"], p["blocks"], p["rows_per_block"], p["empty"]) == ("narrow", 1024, 17, 59) and 0 < p["last_rows"] < 17
    assert _plan("s07a")["kind"] == "narrow" and _plan("s08")["kind"] == "rows"
    p = _plan("s09")
    assert (p["kind"], p["blocks"], p["rows_per_block"], p["empty"], p["last_rows"]) == ("rows", 128, 2, 63, 1)
    assert _plan("s10")["kind"] == "rows" and R.SHAPE["s10"][1] <= 4
    p = _plan("s12a")
    assert (p["kind"], p["blocks"], p["rows_per_block"], p["empty"], p["last_rows"]) == ("mfma", 512, 2, 255, 1)
    assert _plan("s12b")["kind"] == "mfma" and _plan("s11c")["kind"] == "rows" and _plan("s11d")["kind"] == "rows"


def test_shapes_reach_the_predicates():
    e = lambda key: tuple(f(*R.SHAPE[key]) for f in (R.expect_d16, R.expect_norm, R.expect_x16))
    assert e("s01") == e("s02") == e("s04") == e("s05") == e("s06") == (True, True, True)
    assert all(e(k) == (True, True, True) for k in ("s03_co1", "s03_co2", "s03_co3", "s03_co4"))
    assert e("s07a") == e("s07b") == (True, True, False)              # the fold on 32 channels, no bf16-stored input
    assert e("s10") == (True, False, False)                           # cout <= 4 but not narrow: the fold is refused
    assert e("s08") == e("s09") == e("s11a") == e("s11b") == e("s11c") == e("s11d") == e("s13") == (True, False, False)
    assert e("s12a") == e("s12b") == (False, False, False)            # w % 4 != 0: every _d16 / _norm / _x16 entry refuses


def test_shapes_reach_the_tile_map_and_sweep_branches():
    assert R.dgrad_items(R.SHAPE["s06"][2]) == 16400 > 4096 * 4       # the direct data gradient's item sweep loops
    assert all(R.dgrad_items(shp) <= 4096 * 4 for k, _, _, shp in R.SHAPES if k != "s06")
    # x tiles of 64 cells: one full, one full + 8, three
    assert [-(-R.SHAPE[k][2][3] // 64) for k in ("s02", "s03_co3", "s04", "s13")] == [1, 2, 3, 6]
    # per-z forward map (32 channels: one row per group; 3 planes x (yc + 2) rows of w * cin fp32 live)
    fwd_yc = lambda key: R.chunk_rows(R.SHAPE[key][2][3] * R.SHAPE[key][0] * 4, 1, 2, 3)
    assert _chunks(17, fwd_yc("s07a")) == [16, 1]
    assert _chunks(18, fwd_yc("s13")) == [8, 8, 2]
    # data-gradient map (4 planes x (2 yc + 2) rows of 2 w * cout elements live): fp32 and bf16 dout
    dg_yc = lambda key, esize: R.chunk_rows(2 * R.SHAPE[key][2][3] * R.SHAPE[key][1] * esize, 2, 2, 4)
    assert _chunks(17, dg_yc("s07a", 4)) == [16, 1]
    assert (dg_yc("s08", 4), dg_yc("s08", 2)) == (8, 16) and _chunks(9, 8) == [8, 1] and _chunks(9, 16) == [9]
    assert (dg_yc("s13", 4), dg_yc("s13", 2)) == (1, 4) and _chunks(18, 4) == [4, 4, 4, 4, 2]
