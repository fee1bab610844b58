"""The checkers of tests/conv2d_ref.py can fail (no GPU, no native library).  A host emulation of the tile kernels (conv2d_ref.emulate:
parity classes, row tiles, taps, 32-channel sub-steps, fp32 accumulate, one bf16 store, per-tile slabs, the UP scatter) passes every
checker; each seeded defect is rejected by them.

The same defects under the criterion the dense 2-D tests had until now (6e-3 * max|ref| on random normal data at those tests' own
small shapes; for the slab defects the summed-over-tiles statistics check at 1e-3 * max + 1e-2).  On this machine it ACCEPTS
    truncate         truncation instead of round-to-nearest-even
    slab_unrounded   slabs summed from the unrounded accumulator
    row_past_end     a row past m_total written (nothing looked there)
and rejects the defects that corrupt whole rows of a tile (border_tap, edge_wrap, straddle, class_swap, and at these channel counts
substep_dropped / substep_twice: a 32-channel half of one tap is 1/18 of the K loop at cin = 64) or leave slabs at their fill
(slab_index); OLD_ACCEPTS pins that list.
"""
import pytest
import torch

import bn_pass_ref as R
import conv2d_ref as C

OLD_ACCEPTS = {"truncate", "slab_unrounded", "row_past_end"}


def run_emulation(g, mode, seed=0, bias=True, rows=None, defect=None, act=None):
    """-> (plan, ref, ybuf, slabbuf, bnbwd) of the emulated launch on integer operands"""
    amp = 1 if mode == "exact" else 3
    x, w, b = C.int_operands(g, amp, seed, bias and act is None)
    ref = C.reference(g, x, w, b)
    plan = C.emu_plan(g, rows)
    front = C.fence_rows(g)
    xbuf, _ = C.fenced(C.nhwc_rows(x), front, torch.float32, "cpu")
    ybuf, _ = R.poisoned(C.out_pixels(g), g.cout, dtype=C.BF, device="cpu")
    slabbuf, _ = R.poisoned(plan.tiles, 2, g.cout, dtype=torch.float32, device="cpu")
    bnbwd = None
    if act is not None:
        bnbwd = C.bnbwd_operands(C.gemm_rows(g), g.cout, seed + 1) + (act,)
    C.emulate(g, plan.rows, xbuf, front, w, b, ybuf, slabbuf, defect, bnbwd)
    return plan, ref, ybuf, slabbuf, bnbwd


def check(g, mode, **kw):
    plan, ref, ybuf, slabbuf, bnbwd = run_emulation(g, mode, **kw)
    C.check_case(g, plan, mode, ref, ybuf, slabbuf, bnbwd, what=C.KIND_NAMES[g.kind])


CLEAN = [
    (C.geo(C.K3, 2, 13, 11, 64, 128, 1, 1), "exact", {}),
    (C.geo(C.K3, 3, 5, 7, 128, 64, 1, 1), "exact", {"bias": False}),               # the shared-A shape; tiles straddle images
    (C.geo(C.K3, 1, 3, 3, 64, 64, 0, 1), "exact", {}),                             # one output pixel
    (C.geo(C.K3, 2, 9, 8, 64, 128, 1, 2), "exact", {"rows": 64}),
    (C.geo(C.K3, 1, 10, 7, 64, 128, 0, 2), "exact", {"rows": 96}),
    (C.geo(C.K3, 1, 1, 5, 64, 64, 1, 1), "exact", {}),                             # H = 1 with pad 1
    (C.geo(C.K1, 3, 7, 5, 128, 128), "exact", {"rows": 96}),
    (C.geo(C.UP, 3, 5, 3, 128, 128, ks=4), "exact", {"rows": 64}),
    (C.geo(C.UP, 2, 3, 5, 128, 64, ks=3), "exact", {}),
    (C.geo(C.UP, 1, 1, 1, 64, 128, ks=4), "exact", {}),
    (C.geo(C.K4S2, 2, 6, 10, 64, 128), "exact", {}),
    (C.geo(C.K2S2, 2, 7, 9, 64, 128), "exact", {}),
    (C.geo(C.K3, 2, 13, 11, 128, 128, 1, 1), "rounded", {"rows": 96}),
    (C.geo(C.K3_BNBWD, 2, 9, 7, 64, 128, 1, 1), "exact", {"act": 0}),
    (C.geo(C.K3_BNBWD, 2, 9, 7, 64, 128, 1, 1), "exact", {"act": 1, "rows": 64}),
    (C.geo(C.K1_BNBWD, 1, 9, 15, 128, 128), "exact", {"act": 2, "rows": 96}),
]


@pytest.mark.parametrize("g,mode,kw", CLEAN, ids=[f"{C.KIND_NAMES[c[0].kind]}-{i}" for i, c in enumerate(CLEAN)])
def test_the_emulation_passes_every_checker(g, mode, kw):
    check(g, mode, **kw)


def test_the_rounding_set_holds_ties_and_the_exact_set_its_condition():
    g = C.geo(C.K3, 2, 13, 11, 128, 128, 1, 1)
    ref = C.reference(g, *C.int_operands(g, 3, 0, True))
    odd = (ref.abs() > 256) & (ref.abs() < 512) & (ref % 2 != 0)
    assert int(odd.sum()) >= 100                                   # exact bf16 ties: round to even decides them
    assert not torch.equal(C.truncate_bf16(ref.float()).float(), C.rounded(ref).float())
    with pytest.raises(AssertionError, match="max.ref"):
        C.assert_exact_condition(ref)
    g1 = C.geo(C.K3, 2, 13, 11, 256, 256, 1, 1)
    assert C.assert_exact_condition(C.reference(g1, *C.int_operands(g1, 1, 0, True))) <= 256


# defect -> (geometry, mode, keyword arguments of the emulation): the smallest case in which the defect changes something
G3 = C.geo(C.K3, 3, 5, 7, 64, 128, 1, 1)           # m = 105: with 64-row tiles, tile 0 and tile 1 both straddle two images
GUP = C.geo(C.UP, 2, 3, 5, 128, 128, ks=3)
DEFECT_CASES = {
    "border_tap": (G3, "exact", {"rows": 64}),
    "edge_wrap": (G3, "exact", {"rows": 64}),
    "straddle": (G3, "exact", {"rows": 64}),
    "substep_dropped": (G3, "exact", {"rows": 64}),
    "substep_twice": (G3, "exact", {"rows": 64}),
    "truncate": (C.geo(C.K3, 2, 13, 11, 128, 128, 1, 1), "rounded", {}),
    "slab_unrounded": (C.geo(C.K3, 2, 13, 11, 128, 128, 1, 1), "rounded", {}),
    "slab_index": (GUP, "exact", {"rows": 64}),
    "row_past_end": (G3, "exact", {"rows": 64}),
    "class_swap": (GUP, "exact", {"rows": 64}),
}


def test_every_defect_has_a_case():
    assert set(DEFECT_CASES) == set(C.DEFECTS)


@pytest.mark.parametrize("defect", C.DEFECTS)
def test_seeded_defect_is_rejected(defect):
    g, mode, kw = DEFECT_CASES[defect]
    check(g, mode, **kw)                                           # the same case without the defect passes
    with pytest.raises(AssertionError):
        check(g, mode, defect=defect, **kw)


def test_a_wrong_backward_sum_is_rejected():
    """the batch-norm backward checkers: a slab that sums the wrong activation mask (act 1) or drops the g z product's sign (act 2)"""
    g = C.geo(C.K3_BNBWD, 2, 9, 7, 64, 128, 1, 1)
    for act in (1, 2):
        plan, ref, ybuf, slabbuf, bnbwd = run_emulation(g, "exact", act=act)
        z, scale, shift, _ = bnbwd
        C.check_case(g, plan, "exact", ref, ybuf, slabbuf, bnbwd)
        with pytest.raises(AssertionError):
            C.check_case(g, plan, "exact", ref, ybuf, slabbuf, (z, scale, shift + 1.0, act))
        wrong = slabbuf.clone()
        wrong[R.GUARD, 1, 5] += 1.0 if act == 1 else 0.125   # (the GELU bound on a 64-row sum of |g z| ~ 1e3 is ~ 1e-2)
        with pytest.raises(AssertionError):
            C.check_case(g, plan, "exact", ref, ybuf, wrong, bnbwd)


# the old tests' own small shapes: test_dense2d_gpu.CASES[0] / [2], test_conv_s2_gpu (3, 5, 3, 128, 128)
OLD_3X3 = C.geo(C.K3, 3, 33, 9, 64, 128, 1, 1)
OLD_UP = C.geo(C.UP, 3, 5, 3, 128, 128, ks=4)


def old_verdict(defect):
    """does the old criterion accept the emulated defect on random normal data?"""
    g = OLD_UP if defect in ("slab_index", "class_swap") else OLD_3X3
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(g.n, g.cin, g.h, g.w, generator=gen).to(C.BF)
    w = (torch.randn(C.weight_shape(g), generator=gen) * 0.05).to(C.BF).float()
    b = torch.randn(g.cout, generator=gen)
    ref = C.conv64(g, x, w, b)
    plan = C.emu_plan(g, 64)
    front = C.fence_rows(g)
    xbuf, _ = C.fenced(C.nhwc_rows(x), front, torch.float32, "cpu")
    ybuf, y = R.poisoned(C.out_pixels(g), g.cout, dtype=C.BF, device="cpu")
    slabbuf, slabs = R.poisoned(plan.tiles, 2, g.cout, dtype=torch.float32, device="cpu")
    C.emulate(g, plan.rows, xbuf, front, w, b, ybuf, slabbuf, defect)
    return C.old_criterion(y, ref) and C.old_stats_criterion(slabs, y)


def test_the_old_criterion_accepts_the_clean_emulation():
    assert old_verdict(None)


@pytest.mark.parametrize("defect", C.DEFECTS)
def test_what_the_old_criterion_lets_through(defect):
    assert old_verdict(defect) == (defect in OLD_ACCEPTS), defect
    assert "truncate" in OLD_ACCEPTS
