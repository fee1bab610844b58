"""The checkers of tests/conv2d_wgrad_ref.py can fail (no GPU, no native library).  A host emulation of the weight-gradient launch
(conv2d_wgrad_ref.emulate: split ranges, the incremental step walk, A / B tile staging through the NS-slot ring with the range tests and
the zero page, the per-kx row offset, per-split slabs, the four-row fold, the dbias path) passes every checker; each seeded defect is
rejected by them.

The same defects under the criterion the dense weight-gradient tests had until now (1e-3 * max|ref| for the stride-1 entries,
2e-3 * max|ref| for the stride-2 ones and the bias gradient, on random normal data at those tests' own small shapes under the default
plan of a 256-CU device).  Found by running it here, it ACCEPTS
    stale_slot       a ring slot that keeps the tiles of step i - NS: every old small shape gives a workgroup fewer K-steps than the
                     ring has slots (asserted below), so no slot is ever reused and the defect cannot act
    row_past_cout    a slab row written past cout (behind the slabs nothing looked)
and rejects the others: at one to four K-steps per workgroup a dropped or doubled step, a shifted tap or a missing split is a visible
share of every sum.  The old bars were not loose for what those launches ran: they never ran the steady-state ring (only the BEV-size
launches do, where a step is one of 4 512 and the emulation is too slow to say what the bar would see).  OLD_ACCEPTS pins the list.
"""
import pytest
import torch

import bn_pass_ref as R
import conv2d_wgrad_ref as W

OLD_ACCEPTS = {"stale_slot", "row_past_cout"}


def run_emulation(g, splits, deep=True, with_db=True, defect=None, seed=0, operands=None):
    """-> (plan, x, dy, dwbuf, dbbuf, wsbuf) of the emulated launch on integer operands (or the given float64 operands)"""
    plan = W.mirror_plan(g, deep=deep, splits=splits)
    x, dy = W.int_operands(g, seed) if operands is None else operands
    fx, fd = W.fences(g)
    xbuf, _ = W.fenced(W.nhwc_flat(x), fx, torch.float32, "cpu")
    dybuf, _ = W.fenced(W.nhwc_flat(dy), fd, torch.float32, "cpu")
    (dwbuf, _), (dbbuf, _), (wsbuf, _) = W.out_buffers(g, plan, with_db, "cpu")
    W.emulate(g, plan, xbuf, fx, dybuf, fd, dwbuf, dbbuf, wsbuf, defect)
    return plan, x, dy, dwbuf, dbbuf, wsbuf


def check(g, splits, **kw):
    plan, x, dy, dwbuf, dbbuf, wsbuf = run_emulation(g, splits, **kw)
    W.check_case(g, plan, x, dy, dwbuf, dbbuf, wsbuf, what=W.ENTRY_NAMES[W.entry_of(g)])
    return plan


CLEAN = [
    (W.geo(W.K3, 2, 5, 40, 64, 64, 1), 3, {}),                                 # 20 steps, splits of 7, 7, 6: mid-row and mid-image starts
    (W.geo(W.K3, 1, 5, 40, 64, 64, 1), 1, {"deep": False}),                    # 10 steps on the four-slot ring: wraps twice
    (W.geo(W.K3, 2, 3, 35, 128, 64, 0), 2, {"with_db": False}),                # Ho = 1, Wo = 33: a K-step with one live pixel
    (W.geo(W.K3, 2, 1, 33, 64, 128, 1), 4, {}),                                # H = 1 with pad 1: kernel rows 0 and 2 outside the image
    (W.geo(W.K3, 1, 3, 20, 192, 192, 1), 2, {}),                               # 3 x 3 channel tiles
    (W.geo(W.K1, 2, 3, 70, 128, 64), 5, {}),
    (W.geo(W.K1, 1, 1, 1, 64, 64), 1, {"with_db": False}),
    (W.geo(W.S2, 2, 4, 66, 64, 64, ks=3), 3, {"with_db": False}),              # Wo = 33
    (W.geo(W.S2, 1, 2, 2, 64, 128, ks=4), 1, {"with_db": False}),              # Ho = Wo = 1
    (W.geo(W.S2, 2, 6, 64, 128, 64, ks=4), 4, {"with_db": False, "deep": False}),
    (W.geo(W.S2, 1, 12, 8, 128, 128, ks=3), 1, {"with_db": False}),            # NS 5: 6 steps
]


@pytest.mark.parametrize("g,splits,kw", CLEAN, ids=[f"{W.ENTRY_NAMES[W.entry_of(c[0])].replace(' ', '_')}-{i}" for i, c in enumerate(CLEAN)])
def test_the_emulation_passes_every_checker(g, splits, kw):
    check(g, splits, **kw)


def test_the_mirror_knows_the_ring_depths_and_load_counts():
    """WgCfg restated: the four-slot ring is 4 deep everywhere; the deep ring holds 8 slots except where the stride-2 X tile of a
    128-channel tile leaves room for 5 or 6; every wave issues one to four loads per K-step (the four vmcnt cases of the kernel)"""
    deep = {(e, tco, tci): W.cfg(tco, tci, ks, st, True) for e, (ks, st) in enumerate([(3, 1), (1, 1), (3, 2), (4, 2)]) for tco in (64, 128) for tci in (64, 128)}
    assert {k: c.ns for k, c in deep.items() if c.ns != 8} == {(2, 64, 128): 6, (3, 64, 128): 6, (2, 128, 128): 5, (3, 128, 128): 5}
    assert all(W.cfg(tco, tci, ks, st, False).ns == 4 for ks, st in [(3, 1), (1, 1), (3, 2), (4, 2)] for tco in (64, 128) for tci in (64, 128))
    assert all(c.ns * 16 * c.chunks <= W.LDS_BYTES for c in deep.values())
    assert {v for c in deep.values() for v in c.nl} == {1, 2, 3, 4}
    assert deep[(0, 64, 64)].nl == (2, 2, 2, 1, 1, 1, 1, 1) and deep[(3, 128, 128)].nu == 4


def test_the_exact_condition_is_on_the_reference():
    g = W.geo(W.K3, 2, 5, 40, 64, 64, 1)
    ref, _ = W.reference(g, *W.int_operands(g, 0))
    assert 0 < W.assert_exact_condition(g, ref) < 9 * 2 * 5 * 40
    assert len({int(v) for v in ref.flatten()[:64]}) > 8                       # every (co, ci, ky, kx) has its own expected value
    with pytest.raises(AssertionError, match="2\\^24"):
        W.assert_exact_condition(W.geo(W.K1, 4, 700, 700, 64, 64), ref)


# defect -> (geometry, forced splits, keyword arguments of the emulation): the smallest case in which the defect changes something
G10 = W.geo(W.K3, 2, 5, 40, 64, 64, 1)            # 20 steps
DEFECT_CASES = {
    "last_step_dropped": (G10, 3, {}),
    "step_twice": (G10, 3, {}),
    "stale_slot": (W.geo(W.K3, 1, 5, 40, 64, 64, 1), 1, {}),                   # 10 steps on 8 slots: step 8 is the first to reuse a slot
    "kx_off": (G10, 3, {}),
    "pad_column": (G10, 3, {}),
    "outside_row": (W.geo(W.K3, 2, 1, 33, 64, 64, 1), 2, {}),
    "filler": (W.geo(W.K3, 2, 3, 35, 64, 64, 0), 2, {}),
    "s2_stride1": (W.geo(W.S2, 2, 4, 66, 64, 64, ks=3), 3, {"with_db": False}),
    "cot_cit_swapped": (W.geo(W.K3, 1, 3, 20, 64, 192, 1), 2, {}),            # 3 x 1 tiles: the exchanged counts decode ci tiles 1 and 2
    "split_left_out": (G10, 3, {}),
    "dbias_cit1": (W.geo(W.K1, 2, 3, 40, 192, 64), 2, {}),                     # three input-channel tiles
    "row_past_cout": (G10, 3, {"with_db": False}),
}


def test_every_defect_has_a_case():
    assert set(DEFECT_CASES) == set(W.DEFECTS)


@pytest.mark.parametrize("defect", W.DEFECTS)
def test_seeded_defect_is_rejected(defect):
    g, splits, kw = DEFECT_CASES[defect]
    check(g, splits, **kw)                                                     # the same case without the defect passes
    with pytest.raises(AssertionError):
        check(g, splits, defect=defect, **kw)


def test_an_outside_row_or_pad_column_shows_as_nan_or_wrong_integer():
    """what the fences are for: the first image's row -1 lies in the NaN fence, the second image's in the first image"""
    g = W.geo(W.K3, 2, 1, 33, 64, 64, 1)
    plan, x, dy, dwbuf, _, _ = run_emulation(g, 2, defect="outside_row")
    dw = dwbuf[R.GUARD:-R.GUARD].reshape(64, 64, 3, 3)
    assert bool(torch.isnan(dw[:, :, 0]).all()) and bool(torch.isfinite(dw[:, :, 1]).all())
    plan, x, dy, dwbuf, _, _ = run_emulation(W.geo(W.K3, 1, 5, 40, 64, 64, 1), 1, defect="pad_column")
    assert bool(torch.isnan(dwbuf[R.GUARD:-R.GUARD]).any())


# the old tests' own small shapes: test_dense2d_gpu.test_conv3x3_wgrad_matches_float64 (2, 64, 64, 20, 24, pad 1) and (1, 128, 192, 17, 19,
# pad 0), test_conv_s2_gpu.test_stride2_conv3x3_backward (2, 9, 6, 64, 192), test_bias_gradient_rides_on_the_weight_gradient_launch's
# smallest 1x1 (1, 13, 9, 1024 -> 256)
OLD_3X3 = W.geo(W.K3, 2, 20, 24, 64, 64, 1)
OLD_3X3_P0 = W.geo(W.K3, 1, 17, 19, 128, 192, 0)
OLD_S2 = W.geo(W.S2, 2, 18, 12, 64, 192, ks=3)
OLD_1X1 = W.geo(W.K1, 1, 13, 9, 1024, 256)
OLD_SHAPE = {"s2_stride1": OLD_S2, "cot_cit_swapped": OLD_3X3_P0, "pad_column": OLD_3X3_P0, "dbias_cit1": OLD_1X1}


def old_verdict(defect):
    """does the old criterion accept the emulated defect on random normal data, under the default plan of a 256-CU device?"""
    g = OLD_SHAPE.get(defect, OLD_3X3)
    ho, wo = W.out_hw(g)
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(g.n, g.cin, g.h, g.w, generator=gen).to(W.BF).double()
    dy = torch.randn(g.n, g.cout, ho, wo, generator=gen).to(W.BF).double()
    with_db = g.kind != W.S2
    plan, _, _, dwbuf, dbbuf, _ = run_emulation(g, None, with_db=with_db, defect=defect, operands=(x, dy))
    tol = 2e-3 if g.kind == W.S2 else 1e-3
    ok = W.old_criterion(dwbuf[R.GUARD:-R.GUARD].reshape(g.cout, g.cin, g.ks, g.ks), W.wgrad64(g, x, dy), tol)
    if with_db:
        ok = ok and W.old_criterion(dbbuf[R.GUARD:-R.GUARD].reshape(-1), dy.sum((0, 2, 3)), 2e-3)
    return ok, plan


def test_the_old_criterion_accepts_the_clean_emulation_and_never_left_the_prologue():
    ok, plan = old_verdict(None)
    assert ok
    for g in (OLD_3X3, OLD_3X3_P0, OLD_S2, OLD_1X1):
        plan = W.mirror_plan(g)
        assert plan.spb < plan.ns, (g, plan)                                    # prologue-only launches: the ring never wrapped


@pytest.mark.parametrize("defect", W.DEFECTS)
def test_what_the_old_criterion_lets_through(defect):
    assert old_verdict(defect)[0] == (defect in OLD_ACCEPTS), defect
