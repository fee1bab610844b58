"""The checkers of tests/pfn_ref.py can fail, shown on the host: the fp32 emulation of every csrc/pfn.hip entry passes every case of the
tables the GPU suite (tests/test_pfn_parity_gpu.py) runs, and each of eleven planted defects is rejected.  The tables alone are checked
for coverage of every entry of pfn.hip and of every slot count / pillar count edge.  Also confirms, with the float64 reference alone,
that the committed seeds meet the 95 % strict-argmax condition and that the redraw loop of the pfn2_bwd screening empties within its
cap (the counts are printed by the last test)."""
import functools
import os
import re

import pytest
import torch

import pfn_ref as R

SEEDS = {}     # (P, T) -> (redraw rounds, share rejected in the first round, {entry: strict share})
BWD_VARIANTS = (("valid", "train"), ("valid", "eval"), ("n", "train"), ("above_n", "eval"), ("last", "train"), ("zero", "eval"))


@functools.lru_cache(maxsize=None)
def params():
    return R.make_params()


@functools.lru_cache(maxsize=2)
def setup(p, t):
    case = R.screened_case(p, t, params())
    return case, R.Ref1(case, params()), R.Ref2(case, params())


def run_one_layer(case, ref, defect=None, kinds=R.ADVERSARIAL_ARG):
    prm, blocks = params(), R.blocks_mirror(case.P)
    R.check_rows(R.emu_stats(case, prm, blocks, defect), *ref.stats(blocks), "pfn_stats", "emu pfn_stats")
    y, ey = ref.apply()
    out, arg = R.emu_apply_max(case, prm, defect)
    share = R.check_argmax(y, ey, ref.part, out, arg, "pfn_apply_max", "emu pfn_apply_max")
    first = R.first_max(y, ref.part)[1]
    g = R.make_grad(case, 21, "cpu")
    for kind in kinds:
        a = R.make_arg(case, kind, first)
        R.check_bwd_rows(R.emu_bwd(case, prm, a, g, blocks, defect), *ref.bwd(a, g, blocks), f"pfn_bwd, arg {kind}", "emu pfn_bwd")
    return share


def run_two_layers(case, ref, defect=None, variants=BWD_VARIANTS):
    prm, blocks = params(), R.blocks_mirror(case.P)
    R.check_rows(R.emu_stats1(case, prm, blocks, defect), *ref.stats1(blocks), "pfn2_stats1", "emu pfn2_stats1")
    R.check_rows(R.emu_stats2(case, prm, blocks, defect), *ref.stats2(blocks), "pfn2_stats2", "emu pfn2_stats2")
    y, ey = ref.apply()
    out, arg, h2max = R.emu_apply_max2(case, prm, defect)
    share = R.check_argmax(y, ey, ref.part, out, arg, "pfn2_apply_max", "emu pfn2_apply_max", ref.h2, ref.eh2, h2max)
    first = R.first_max(y, ref.part)[1]
    g = R.make_grad(case, 22, "cpu")
    for kind, abd in variants:
        a = R.make_arg(case, kind, first)
        rows = R.emu_bwd2(case, prm, a, g, prm.abd2[abd], defect)
        R.check_bwd_rows(rows, *ref.bwd(a, g, prm.abd2[abd]), f"pfn2_bwd, arg {kind}, abd2 {abd}", "emu pfn2_bwd")
    return share


@pytest.mark.parametrize("p,t", R.CASES)
def test_clean_emulation_passes_every_case(p, t):
    case, ref1, ref2 = setup(p, t)
    s1 = run_one_layer(case, ref1)
    s2 = run_two_layers(case, ref2)
    SEEDS[(p, t)] = (case.rounds, case.first_reject, {"pfn_apply_max": s1, "pfn2_apply_max": s2})


def test_planted_content_is_there():
    """the planted content of a mid-sized case: every forced num_points value, exact ties, maxima in an empty slot of a pillar with
    points, negative scales and all-zero channels where slot 0 wins"""
    case, ref1, ref2 = setup(1025, 13)
    t = case.T
    for v in (0, 1, t, t + 3, -1):
        assert int((case.num == v).sum()) >= 10, v
    prm = params()
    for y, part, scale, shift in ((ref1.apply()[0], ref1.part, prm.scale, prm.shift), (ref2.apply()[0], ref2.part, prm.ss2[:R.C], prm.ss2[R.C:])):
        top, first, gap = R.first_max(y, part)
        n = ref1.n[:, None].expand_as(first)
        assert int(((gap == 0) & (top > 0) & (n >= 2)).sum()) >= 100, "exact ties of positive maxima (duplicated points)"
        assert int(((first == n) & (n >= 1) & (n < t)).sum()) >= 100, "maxima in the empty slot of a pillar with points"
        assert int((scale < 0).sum()) >= 8 and int((shift > 0).sum()) == shift.numel() // 2
        for z in R.ZERO_CHANNELS:
            assert bool((y[:, :, z] == 0).all()) and bool((first[:, z] == 0).all())
    assert bool((ref2.x1[:, :, R.ZERO_CHANNELS[0]] == 0).all())


# (defect, reader, P, T, the checker that must reject it: a pattern of its message)
DEFECT_CASES = [
    ("skip_last_of_second_trip", "one", 4097, 13, r"^pfn_stats: "), ("skip_last_of_second_trip", "two", 4097, 13, r"^pfn2_stats1: "),
    ("skip_last_of_second_trip", "two", 1025, 13, r"^pfn2_bwd, .*dW2: "),      # 257 blocks: no second trip but in the backward's 1024 waves
    ("pillar_dealt_twice", "one", 5, 13, r"^pfn_stats: "), ("pillar_dealt_twice", "two", 4097, 20, r"^pfn2_stats1: "),
    ("empty_multiplicity_minus_1", "two", 5, 13, r"^pfn2_stats2: "), ("empty_multiplicity_minus_1", "two", 1025, 20, r"^pfn2_stats2: "),
    ("empty_row_left_out", "two", 5, 12, r"^pfn2_stats2: "),
    ("last_maximum", "one", 5, 13, r"^pfn_apply_max: arg is not the FIRST maximum"),
    ("last_maximum", "two", 1025, 13, r"^pfn2_apply_max: arg is not the FIRST maximum"),
    ("m3_zero", "one", 1025, 13, r"^pfn_bwd, .*M3: "), ("m3_zero", "two", 4097, 20, r"^pfn2_bwd, .*M3: "),
    ("upper_columns_not_zeroed", "two", 5, 13, r"^pfn2_bwd, .*sum g: .*\[0, 3[2-9]\]"),      # the first miss sits in columns 32..63
    ("column_counted_twice", "two", 1025, 13, r"^pfn2_bwd, .*sum g h: "),
    ("idle_row_unwritten", "two", 1023, 13, r"^pfn2_bwd, .*dW2: .*\[1023, 0\]"),
    ("num_not_clamped", "one", 5, 13, r"^pfn_stats: "), ("num_not_clamped", "two", 5, 20, r"^pfn2_stats1: "),
    ("centre_x_from_y", "one", 5, 13, r"^pfn_stats: "), ("centre_x_from_y", "two", 1025, 13, r"^pfn2_stats1: "),
]


@pytest.mark.parametrize("defect,reader,p,t,message", DEFECT_CASES)
def test_defect_is_rejected(defect, reader, p, t, message):
    case, ref1, ref2 = setup(p, t)
    with pytest.raises(AssertionError, match=message):
        if reader == "one":
            run_one_layer(case, ref1, defect, kinds=("valid",))
        else:
            run_two_layers(case, ref2, defect, variants=BWD_VARIANTS[:1])


def test_every_defect_has_a_case():
    assert {c[0] for c in DEFECT_CASES} == set(R.DEFECTS)


BACKWARD_SECTION = {"m3_zero": r"^pfn2_bwd, M3: ", "skip_last_of_second_trip": r"^pfn2_bwd, dW2: ", "column_counted_twice": r"^pfn2_bwd, sum g h: ",
                    "empty_multiplicity_minus_1": r"^pfn2_bwd, dW2: "}


@pytest.mark.parametrize("defect", sorted(BACKWARD_SECTION))
def test_defect_is_rejected_by_the_backward_check_itself(defect):
    """the sums-side defects, fed to the backward checker alone (the forward checks above would already have stopped them)"""
    case, _, ref2 = setup(1025, 13)
    prm = params()
    first = R.first_max(ref2.apply()[0], ref2.part)[1]
    g = R.make_grad(case, 22, "cpu")
    a = R.make_arg(case, "valid", first)
    ref, bound = ref2.bwd(a, g, prm.abd2["train"])
    R.check_bwd_rows(R.emu_bwd2(case, prm, a, g, prm.abd2["train"]), ref, bound, "pfn2_bwd", None)
    with pytest.raises(AssertionError, match=BACKWARD_SECTION[defect]):
        R.check_bwd_rows(R.emu_bwd2(case, prm, a, g, prm.abd2["train"], defect), ref, bound, "pfn2_bwd", None)


def test_tables_cover_every_entry_and_edge():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sparse2dense_amd", "csrc", "pfn.hip")
    with open(src) as fh:
        exported = set(re.findall(r'extern "C" \w+ (s2d_pfn\w+)\(', fh.read()))
    assert len(exported) == 13 and exported == R.table_entries()
    assert set(R.T_AXIS) == {1, 2, 12, 13, 19, 20}      # 12 | 13: slots * 5 = 64, the lane boundary of pfn2_fetch; 1; the full pillar
    assert 12 * 5 < 64 <= 13 * 5 and max(R.T_AXIS) == R.T_MAX
    assert set(R.P_AXIS) == {1, 3, 4, 5, 1023, 1025, 4096, 4097, 9001}
    cases = set(R.CASES)
    for p in R.P_AXIS:
        assert (p, 13) in cases and (p, 20) in cases
    for t in R.T_AXIS:
        assert (5, t) in cases and (4097, t) in cases
    assert R.blocks_mirror(4096) == 1024 and R.blocks_mirror(4097) == 1024 and R.blocks_mirror(3) == 1 and R.blocks_mirror(5) == 2
    assert {k for k, _ in BWD_VARIANTS} == set(R.ADVERSARIAL_ARG) and {a for _, a in BWD_VARIANTS} == set(R.ABD2)


@pytest.mark.parametrize("t", [2, 13, 20])
def test_redraw_loop_empties_at_the_module_test_size(t):
    case = R.screened_case(4101, t, params())
    assert 1 <= case.rounds <= R.REDRAW_ROUNDS
    SEEDS[(4101, t)] = (case.rounds, case.first_reject, {})


def test_print_seed_report(capsys):
    with capsys.disabled():
        print("\n   P   T  redraw rounds  rejected in round 1  strict share (pfn_apply_max, pfn2_apply_max)")
        for (p, t), (rounds, rej, shares) in sorted(SEEDS.items()):
            print(f"{p:5d} {t:3d} {rounds:8d} {rej:18.3f}        " + "  ".join(f"{v:.4f}" for v in shares.values()))
