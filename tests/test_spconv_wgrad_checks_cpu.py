"""The checking code of tests/test_spconv_wgrad_parity_gpu.py, run on the host: a small emulation of the weight gradient's split / reduce
structure (driven by R.mirror_plan and R.block_of, the restatements of wgrad_plan and wgrad_block) produces what a launch leaves in the
caller-owned buffers; a right launch passes the checks, each seeded defect is rejected.  No library call.

The premise of the exact suite, as assertions: on the same data the older tests' bound max|dW - ref| <= 2e-3 * max|ref| ACCEPTS a dropped
pair, a pair replaced by rows (0, 0) and a pair counted twice.  How much that bound admits depends on the size: a wrong pair moves an
element by a product of two row entries while max|ref| grows with the square root of the pair count, so with a few thousand pairs per offset
the bound still sees a pair of large rows and misses one of small rows; from roughly 10^5 pairs per offset - the benchmark's row counts -
it misses every single pair.  The problem below has 6 * 10^5 pairs per offset so that the statement holds for ANY pair (asserted, not
assumed: 2e-3 * max|ref| exceeds the largest possible change, 18).
"""
import functools

import pytest
import torch

import spconv_wgrad_ref as R
import test_spconv_wgrad_parity_gpu as G

KVOL, CIN, COUT, N_IN, N_OUT = 3, 16, 16, 2000, 600000
MODE = 0   # the fp32 entry's plan: 170 workgroup rows (no multiple of 8: wgrad_block's plain branch) of 4 wave rows each


@functools.lru_cache(maxsize=None)
def _problem():
    feat, dout, _, _ = R.exact_operands(N_IN, N_OUT, CIN, COUT, 11)
    nbr = R.dense_map(KVOL, N_IN, N_OUT, 11)
    plan = R.mirror_plan(MODE, N_OUT, KVOL, CIN, COUT)
    assert plan["grid_y"] % 8 != 0 and plan["wrow"] == 4 and plan["rows_per_split"] % 32 != 0
    return feat, dout, nbr, plan, R.exact_reference(feat, dout, nbr)


WHERE = (1, 77)   # the (offset, split) a defect is seeded in
T = 40            # ... and the pair


def emulate(defect=None):
    """-> (dbuf, dweight, wbuf, n_partial) after an emulated launch: every workgroup of the kvol x grid_y grid decodes its (offset, row
    block), each of its wave rows sums the pairs of its split - in chunks of 32, which matters to the stale-chunk defect only - and stores
    the partial; a fixed-order fold over the splits gives dweight.  Stores that fall outside the allocation are dropped (a fault on the
    device), stores into the guards land there."""
    from test_spconv_plans_gpu import GUARD
    feat, dout, nbr, plan, _ = _problem()
    n_split, rps, grid_y, wrow = plan["n_split"], plan["rows_per_split"], plan["grid_y"], plan["wrow"]
    per, size = CIN * COUT, KVOL * CIN * COUT
    ws_bytes = R.ceil_div(n_split * size * 4, 256) * 256
    dbuf, dw, wbuf, ws = R.alloc_buffers(ws_bytes, KVOL, CIN, COUT, "cpu")
    flat, base = wbuf.view(-1), GUARD * R.WS_ROW
    for by in range(grid_y):
        for bx in range(KVOL):
            k, rb = R.block_of(bx, by, KVOL, grid_y, swapped=defect == "remap_swapped")
            for w in range(wrow):
                split = rb * wrow + w
                r_begin = split * rps
                r_end = min(N_OUT, r_begin + rps)
                o = torch.arange(r_begin, max(r_end, r_begin))
                j = nbr[k, r_begin:max(r_end, r_begin)].long()
                o, j = o[j >= 0], j[j >= 0]
                if (k, split) == WHERE:
                    if defect == "dropped":
                        o, j = torch.cat([o[:T], o[T + 1:]]), torch.cat([j[:T], j[T + 1:]])
                    elif defect == "zero_zero":
                        o, j = o.clone(), j.clone()
                        o[T] = j[T] = 0
                    elif defect == "doubled":
                        o, j = torch.cat([o, o[T:T + 1]]), torch.cat([j, j[T:T + 1]])
                    elif defect == "stale_chunk":   # the last chunk holds cnt < 32 pairs; slots cnt .. 31 still hold the previous chunk's rows
                        cnt, full = o.numel() % 32, o.numel() // 32
                        assert 0 < cnt and full >= 1
                        stale = slice(32 * (full - 1) + cnt, 32 * full)
                        o, j = torch.cat([o, o[stale]]), torch.cat([j, j[stale]])
                    elif defect == "not_stored":
                        continue
                acc = feat[j].t() @ dout[o]   # fp32, exact
                if defect == "transposed" and (k, split) == WHERE:
                    acc = acc.t().contiguous()
                at = base + (split * KVOL + k) * per
                if 0 <= at and at + per <= flat.numel():
                    flat[at:at + per] = acc.flatten()
    dw.copy_(ws.flatten()[:n_split * size].view(n_split, KVOL, CIN, COUT).sum(0))
    return dbuf, dw, wbuf, n_split * size


def _old_check(dw, ref):
    """tests/test_s16_gpu.py::test_s16_wgrad and test_sparse_weight_gradient_at_benchmark_row_counts"""
    return bool((dw.double() - ref.double()).abs().max() <= 2e-3 * ref.abs().max())


def _rejected(dbuf, dw, wbuf, n_partial, ref):
    try:
        R.check_buffers(dbuf, wbuf, n_partial)
        R.assert_exact(dw, ref)
    except AssertionError as e:
        return str(e.args[0])
    return None


def test_checks_accept_a_correct_launch():
    ref = _problem()[4]
    dbuf, dw, wbuf, n_partial = emulate()
    assert _rejected(dbuf, dw, wbuf, n_partial, ref) is None
    assert _old_check(dw, ref)


@pytest.mark.parametrize("defect", ["dropped", "zero_zero", "doubled"])
def test_one_wrong_pair_fails_the_exact_check_and_passes_the_older_bound(defect):
    """one pair of one (offset, split) dropped / replaced by rows (0, 0) - the r04 race of the cooperative kernel's ring - / read twice - a
    ring slot consumed before it was overwritten"""
    ref = _problem()[4]
    assert 2e-3 * float(ref.abs().max()) > 18   # the largest change a pair of {-3..3} rows can make: 9, or 18 when it is replaced
    dbuf, dw, wbuf, n_partial = emulate(defect)
    R.check_buffers(dbuf, wbuf, n_partial)   # written, finite, inside its buffers: only the comparison can see it
    msg = _rejected(dbuf, dw, wbuf, n_partial, ref)
    assert msg is not None and "differs from the exact reference" in msg
    assert 0 < float((dw.double() - ref.double()).abs().max()) <= 18
    assert _old_check(dw, ref), "the 2e-3 * max|ref| bound of the existing tests was expected to accept this"


def test_unmasked_last_chunk_fails_the_exact_check():
    ref = _problem()[4]
    msg = _rejected(*emulate("stale_chunk"), ref)
    assert msg is not None and "differs from the exact reference" in msg


def test_split_that_stored_nothing_fails_the_workspace_check():
    """its partial stays at the NaN fill: dweight is not finite, and had the reduction skipped it, the workspace check would still see it"""
    ref = _problem()[4]
    dbuf, dw, wbuf, n_partial = emulate("not_stored")
    with pytest.raises(AssertionError, match="rows left at the NaN fill"):
        R.check_buffers(dbuf, wbuf, n_partial)
    dw.copy_(ref.float())   # a reduction that happened to skip the split
    with pytest.raises(AssertionError, match="partial sums left at the NaN fill"):
        R.check_buffers(dbuf, wbuf, n_partial)


def test_swapped_remap_branches_fail():
    """the XCD decode on a grid_y that is no multiple of 8 is no bijection: some (offset, split) are computed twice or stored outside the
    workspace, others never"""
    ref = _problem()[4]
    assert _rejected(*emulate("remap_swapped"), ref) is not None


def test_transposed_store_fails_the_exact_check():
    ref = _problem()[4]
    msg = _rejected(*emulate("transposed"), ref)
    assert msg is not None and "differs from the exact reference" in msg


def test_store_past_the_workspace_fails_the_guard_check():
    from test_spconv_plans_gpu import GUARD
    ref = _problem()[4]
    dbuf, dw, wbuf, n_partial = emulate()
    wbuf[-GUARD, 0] = 0.0
    with pytest.raises(AssertionError, match="workspace: back guard rows overwritten"):
        R.check_buffers(dbuf, wbuf, n_partial)
    dbuf, dw, wbuf, n_partial = emulate()
    dbuf.view(torch.int32)[GUARD - 1, 0, 0] ^= 1
    with pytest.raises(AssertionError, match="dweight: front guard rows overwritten"):
        R.check_buffers(dbuf, wbuf, n_partial)
    assert _rejected(dbuf, dw, wbuf, n_partial, ref) is not None


def test_poisoned_row_reaching_a_sum_fails():
    """an input row no pair names is NaN in the parity cases: a clamped gather whose select is missing puts it into dweight"""
    case = R.exact_case("one_pair", 3, 50, 100, 16, 16, 1)
    assert bool(torch.isnan(case["feat32"][0]).all()) and bool(torch.isnan(case["dout32"][0]).all())
    dw = case["ref"].float() + 0.0 * case["feat32"][0, 0] * case["dout32"][0, 0]
    with pytest.raises(AssertionError, match="differs from the exact reference"):
        R.assert_exact(dw, case["ref"])
    R.assert_exact(case["ref"].float(), case["ref"])


# ---- the reference and the plan restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,p", [("density", 0.5), ("dense", 1.0), ("window_gaps", 1.0), ("last_row", 0.0), ("one_pair", 0.0), ("empty", 0.0)])
def test_exact_reference_is_the_integer_matmul(kind, p):
    kvol, n_in, n_out, cin, cout = 5, 60, 333, 16, 24
    for seed in (1, 2):
        case = R.exact_case(kind, kvol, n_in, n_out, cin, cout, seed, p)
        feat, dout, _, _ = R.exact_operands(n_in, n_out, cin, cout, 7919 * seed + cin + cout)
        nbr = case["nbr"]
        want = torch.zeros(kvol, cin, cout, dtype=torch.int64)
        for k in range(kvol):
            for o in torch.nonzero(nbr[k] >= 0).flatten().tolist():
                want[k] += feat[nbr[k, o]].long().view(-1, 1) * dout[o].long().view(1, -1)
        assert torch.equal(case["ref"], want)
        # the poisoned copies equal the clean operands on every row a pair names and are NaN elsewhere
        used = torch.zeros(n_in, dtype=torch.bool)
        used[nbr[nbr >= 0].long()] = True
        assert torch.equal(case["feat32"][used], feat[used]) and bool(torch.isnan(case["feat32"][~used]).all())
        has = (nbr >= 0).any(0)
        assert torch.equal(case["dout32"][has], dout[has]) and bool(torch.isnan(case["dout32"][~has]).all())
        assert torch.equal(case["feat16"][used].float(), feat[used]) and torch.equal(case["dout16"][has].float(), dout[has])


def test_exact_operands_refuse_row_counts_that_could_round():
    with pytest.raises(AssertionError, match="2\\^24"):
        R.exact_operands(10, R.MAX_ROWS, 16, 16, 0)


def test_mirror_plan_invariants():
    shapes = R.SHAPES16 + [(ci, co) for ci, co, _ in R.VALU_SHAPES]
    for hooks in G.HOOK_SETTINGS:
        for mode in (0, 1, 2):
            for cin, cout in shapes:
                for kvol in R.GRID_KVOL:
                    for n_out in R.GRID_N_OUT + R.CHOICE_ROWS:
                        p = R.mirror_plan(mode, n_out, kvol, cin, cout, **hooks)
                        what = (mode, n_out, kvol, cin, cout, hooks, p)
                        assert p["n_split"] * p["rows_per_split"] >= n_out, what
                        assert p["rows_per_split"] % 4 == 0 and p["rows_per_split"] > 0, what
                        assert p["n_split"] % p["wrow"] == 0 and p["grid_y"] * p["wrow"] == p["n_split"] and p["grid_y"] >= 1, what
                        assert p["n_split"] <= max(R.ceil_div(n_out, 256), p["wrow"]), what
                        # every (offset, split) is owned by exactly one workgroup, whichever branch wgrad_block takes
                        if n_out in (5, 4097) and kvol != 27:
                            owners = sorted(R.block_of(bx, by, kvol, p["grid_y"]) for by in range(p["grid_y"]) for bx in range(kvol))
                            assert owners == [(k, b) for k in range(kvol) for b in range(p["grid_y"])], what


def test_every_split_plan_case_of_the_parity_suite_is_reachable(capsys):
    """the (family, shape, property, kvol) cases of section C, chosen with the mirror as the GPU test chooses them with the library's query;
    prints the table (pytest -s)"""
    rows = []
    for fam, (cin, cout), prop, kvol in G._c_cases():
        entry, hooks, kernel, _, _, _ = G.C_FAMILIES[fam]
        chosen = R.choose_plan(lambda n, w: R.mirror_plan(R.ENTRIES[entry], n, kvol, cin, cout, waves=w, **hooks), prop, kvol)
        assert chosen is not None, (fam, cin, cout, prop, kvol)
        n_out, waves, plan = chosen
        assert n_out <= 20000 and plan["kernel"] == kernel
        rows.append((fam, f"{cin}->{cout}", kvol, prop, n_out, dict(hooks, waves=waves), tuple(plan.values())))
    for r in rows:
        print(*r)
    # what the suite leaves out cannot be had: the transpose-read kernel's grid_y, once 8, is a multiple of 8
    for cin, cout in ((16, 16), (128, 128)):
        assert R.choose_plan(lambda n, w: R.mirror_plan(2, n, 27, cin, cout, waves=w, tr=1), "grid_odd", 27) is None
