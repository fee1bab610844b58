"""The checkers, references and plan mirrors of tests/bn_pass_ref.py, run on the host: a faithful emulation of every operation (torch fp32
arithmetic, bf16 round-to-nearest stores) passes each checker at a small shape of each family, and each of eight seeded defects is
rejected by the checker meant for it.  No library call."""
import pytest
import torch

import bn_pass_ref as R

BF, F32 = torch.bfloat16, torch.float32


def _case(c, n, dtype=BF, seed=0):
    g = torch.Generator().manual_seed(seed + 100 * c + n)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = (rn(n, c) * 2.0 + 0.3).to(dtype)
    scale, shift = rn(c) * 0.5 + 1.0, rn(c) * 0.5
    x[:, 1], scale[1], shift[1] = 1.0, 1.0, -1.0         # exact zeros of z
    scale[2] = 0.0
    if c > 4:
        scale[4] = 5.0                                     # |z| up to 10 and beyond
    dy, res = rn(n, c).to(dtype), rn(n, c).to(dtype)
    y = rn(n, c).clamp_min(0.0).to(dtype)
    a, b, d = rn(c), rn(c) * 0.1, rn(c) * 0.1
    gamma, beta, rm, rv = rn(c) * 0.5 + 1.0, rn(c), rn(c), torch.rand(c, generator=g) + 0.5
    assert R.make_unambiguous(x, scale, shift) == 0
    return dict(x=x, scale=scale, shift=shift, dy=dy, res=res, y=y, a=a, b=b, d=d, gamma=gamma, beta=beta, rm=rm, rv=rv, c=c, n=n)


ROW = (24, R.row_plan_bf16(1, 24).lanes + 1)          # A: one idle thread per workgroup, a ragged second row per lane
BN1D = (16, R.red_plan(1, 16).lanes + 1)              # B
CM = (3, 3, 1020)                                      # C
PART = (257, 16)                                       # D


# ---- faithful emulations pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,shape", [(BF, ROW), (F32, BN1D)])
def test_elementwise_checkers_accept_the_emulation(dtype, shape):
    k = _case(*shape, dtype=dtype)
    for res in (None, k["res"]):
        for act in (0, 1, 2):
            ref, mag, term = R.ref_apply(k["x"], k["scale"], k["shift"], res, act)
            R.check_elementwise(R.emu_apply(k["x"], k["scale"], k["shift"], res, act, dtype), ref, mag, term)
    z, _ = R.ref_z(k["x"], k["scale"], k["shift"])
    for act, y in ((0, None), (1, None), (1, k["y"]), (2, None)):
        g, gerr = R.ref_g(k["dy"], act, z=z, y=y)
        ge = R.emu_g(k["dy"], k["x"], k["scale"], k["shift"], act, y)
        ref, mag, term = R.ref_bwd_apply(g, gerr, k["x"], k["a"], k["b"], k["d"])
        R.check_elementwise(R.emu_bwd_apply(ge, k["x"], k["a"], k["b"], k["d"], dtype), ref, mag, term)
        if act == 2:
            R.check_elementwise(ge.to(dtype), g, g.abs(), gerr)
        else:
            R.check_bits(ge.to(dtype), g.to(dtype))


def _emu_sums(t0, t1, plan):
    return torch.cat([R.emu_block_partials(t0, plan).sum(0), R.emu_block_partials(t1, plan).sum(0)])


@pytest.mark.parametrize("dtype,shape,planner", [(BF, ROW, R.row_plan_bf16), (F32, BN1D, R.red_plan)])
def test_sum_and_finalize_checkers_accept_the_emulation(dtype, shape, planner):
    c, n = shape
    k = _case(c, n, dtype=dtype)
    plan = planner(n, c)
    xf = k["x"].float()
    st = _emu_sums(xf, xf * xf, plan)
    ref, mag = R.ref_sums(k["x"])
    chain = R.chain_rows(plan, R.fold_finalize)
    bound = R.check_sums(st, ref, mag, chain)
    for eps in (1e-3, 1e-5):
        e32 = float(torch.tensor(eps, dtype=F32))
        dev = R.emu_fwd_finalize(st[:c], st[c:], n, k["gamma"], k["beta"], e32, 0.1, k["rm"], k["rv"])
        fn = lambda s0, s1: R.fwd_finalize(s0, s1, n, k["gamma"], k["beta"], e32, float(torch.tensor(0.1, dtype=F32)), k["rm"], k["rv"])
        R.check_box(dev, fn, ref[:c], bound[:c], ref[c:], bound[c:])
    mean, invstd = dev["mean"], dev["invstd"]
    z, _ = R.ref_z(k["x"], k["scale"], k["shift"])
    for act in (0, 1, 2):
        g, gerr = R.ref_g(k["dy"], act, z=z)
        ge = R.emu_g(k["dy"], k["x"], k["scale"], k["shift"], act)
        st = _emu_sums(ge, ge * xf, plan)
        ref, mag, act_sum = R.ref_bwd_sums(g, gerr, k["x"])
        bound = R.check_sums(st, ref, mag, chain, act_sum)
        dev = R.emu_bwd_finalize(st[:c], st[c:], st[:c], st[c:], n, k["gamma"], mean, invstd)

        def fn(s0, s1):
            out = R.bwd_finalize_local(s0, s1, mean, invstd)
            out.update(R.bwd_finalize_global(s0, s1, n, k["gamma"], mean, invstd))
            return out
        R.check_box(dev, fn, ref[:c], bound[:c], ref[c:], bound[c:])


def test_channel_major_and_partial_list_checkers_accept_the_emulation():
    batch, c, pos = CM
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(batch, c, pos, generator=g) * 2 + 0.3, torch.randn(batch, c, pos, generator=g)
    v = lambda t: t.view(1, c, 1)
    scale, shift, a, b, d = (torch.randn(c, generator=g) for _ in range(5))
    assert R.make_unambiguous(x, v(scale), v(shift)) == 0
    plan = R.cm_plan(batch, c, pos)
    for store in (F32, BF):
        xs, dys = x.to(store), dy.to(store)
        assert R.make_unambiguous(xs, v(scale), v(shift)) == 0
        z, _ = R.ref_z(xs, v(scale), v(shift))
        gr, gerr = R.ref_g(dys, 1, z=z)
        ge = R.emu_g(dys, xs, v(scale), v(shift), 1)
        ref, mag, term = R.ref_bwd_apply(gr, gerr, xs, v(a), v(b), v(d))
        R.check_elementwise(R.emu_bwd_apply(ge, xs, v(a), v(b), v(d), store), ref, mag, term, names="sample, channel, position")
        st = torch.cat([ge.sum((0, 2)), (ge * xs.float()).sum((0, 2))])
        ref, mag, _ = R.ref_bwd_sums(gr, gerr, xs, (0, 2))
        R.check_sums(st, ref, mag, R.chain_cm(batch, plan))
    nblocks, c = PART
    part = torch.cat([64 * (0.3 + 0.25 * torch.randn(nblocks, c, generator=g)), 64 * (4.1 + 0.3 * torch.rand(nblocks, c, generator=g))], 1)
    R.check_sums(part.sum(0), part.double().sum(0), part.double().abs().sum(0), R.chain_partials(nblocks, c, True, R.fold_finalize))


# ---- the eight seeded defects --------------------------------------------------------------------------------------------------------------
def _apply_launch(k, act=1, ld=None):
    c, n = k["c"], k["n"]
    ref, mag, term = R.ref_apply(k["x"], k["scale"], k["shift"], None, act)
    buf, y, off = R.wide(n, c, ld or c, BF, "cpu")
    y.copy_(R.emu_apply(k["x"], k["scale"], k["shift"], None, act, BF))
    return buf, y, off, ref, mag, term


def test_defect_1_last_row_of_a_ragged_tail_left_at_the_fill():
    k = _case(*ROW)
    buf, y, off, ref, mag, term = _apply_launch(k)
    R.assert_slice_written(buf, off, k["c"], "y")
    R.check_elementwise(y, ref, mag, term)
    y[-1] = float("nan")
    with pytest.raises(AssertionError, match="left at the NaN fill"):
        R.assert_slice_written(buf, off, k["c"], "y")
    with pytest.raises(AssertionError, match=rf"\[\[{k['n'] - 1}, 0\]"):
        R.check_elementwise(y, ref, mag, term)


def test_defect_2_a_channel_group_with_its_neighbours_scale():
    k = _case(*ROW)
    ref, mag, term = R.ref_apply(k["x"], k["scale"], k["shift"], None, 0)
    wrong = k["scale"].clone()
    wrong[8:16] = k["scale"][0:8]
    y = R.emu_apply(k["x"], wrong, k["shift"], None, 0, BF)
    with pytest.raises(AssertionError, match=r"first \(row, channel\): \[\[0, (8|9|10)\]"):
        R.check_elementwise(y, ref, mag, term)


def test_defect_3_bf16_truncation_passes_the_old_criterion_and_fails_the_new_one():
    k = _case(136, 4099)
    ref, mag, term = R.ref_apply(k["x"], k["scale"], k["shift"], None, 0)
    v = k["x"].float() * k["scale"] + k["shift"]
    rounded = v.to(BF)
    truncated = (v.view(torch.int32) & -65536).view(F32).to(BF)
    R.check_elementwise(rounded, ref, mag, term)
    assert R.old_criterion(rounded, ref) and R.old_criterion(truncated, ref), "the per-tensor 1e-2 * max|ref| criterion accepts both"
    with pytest.raises(AssertionError, match="outside the bound"):
        R.check_elementwise(truncated, ref, mag, term)
    missed = ((truncated.double() - ref).abs() > 0.5 * R.ulp_bf16(ref) + 4 * R.ulp_fp32(mag)).double().mean()
    assert 0.3 < float(missed) < 0.7, float(missed)   # about half of all elements


def test_defect_4_the_fold_drops_the_last_workgroups_partial_row():
    c = 24
    lanes = R.row_plan_bf16(1, c).lanes
    n = 2 * lanes * R.ROW_RPT + 3 * lanes + 1
    k = _case(c, n)
    plan = R.row_plan_bf16(n, c)
    assert plan.nblocks == 3 and plan.empty == 0
    xf = k["x"].float()
    p0, p1 = R.emu_block_partials(xf, plan), R.emu_block_partials(xf * xf, plan)
    ref, mag = R.ref_sums(k["x"])
    chain = R.chain_rows(plan, R.fold_sum)
    R.check_sums(torch.cat([p0.sum(0), p1.sum(0)]), ref, mag, chain)
    with pytest.raises(AssertionError, match="sums outside"):
        R.check_sums(torch.cat([p0[:-1].sum(0), p1[:-1].sum(0)]), ref, mag, chain)


def test_defect_5_mask_of_greater_or_equal_on_the_exact_zeros():
    k = _case(*ROW)
    z, _ = R.ref_z(k["x"], k["scale"], k["shift"])
    assert bool((z[:, 1] == 0).all()) and int(R.ambiguous(k["x"], k["scale"], k["shift"]).sum()) == 0
    g, gerr = R.ref_g(k["dy"], 1, z=z)
    ref, mag, term = R.ref_bwd_apply(g, gerr, k["x"], k["a"], k["b"], k["d"])
    zf = k["x"].float() * k["scale"] + k["shift"]
    wrong = torch.where(zf >= 0, k["dy"].float(), torch.zeros(()))
    with pytest.raises(AssertionError, match=r"bit comparison.*\[\[0, 1\]"):
        R.check_bits(wrong.to(BF), g.to(BF), "dres")
    with pytest.raises(AssertionError, match=r"\[\[0, 1\]"):
        R.check_elementwise(R.emu_bwd_apply(wrong, k["x"], k["a"], k["b"], k["d"], BF), ref, mag, term)


def test_defect_6_a_strided_store_at_row_stride_c():
    k = _case(*ROW)
    c, n = ROW
    for ld in (c + 8, 3 * c):
        buf, y, off, ref, mag, term = _apply_launch(k, ld=ld)
        R.assert_slice_written(buf, off, c, "y")
        good = y.clone()
        buf.fill_(float("nan"))
        flat = buf[R.GUARD:].reshape(-1)
        start = off
        flat[start:start + n * c] = good.reshape(-1)            # rows packed at stride c from the slice's first element
        with pytest.raises(AssertionError, match="outside the destination slice"):
            R.assert_slice_written(buf, off, c, "y")


def _finalize_inputs():
    c, n = ROW
    k = _case(c, n)
    ref, mag = R.ref_sums(k["x"])
    d = R.chain_rows(R.row_plan_bf16(n, c), R.fold_finalize) * R.U32 * mag
    return k, c, n, ref, d


def test_defect_7_running_var_updated_with_the_biased_variance():
    k, c, n, ref, d = _finalize_inputs()
    st = ref.float()
    fn = lambda s0, s1: R.fwd_finalize(s0, s1, n, k["gamma"], k["beta"], 1e-3, 0.1, k["rm"], k["rv"])
    dev = R.emu_fwd_finalize(st[:c], st[c:], n, k["gamma"], k["beta"], 1e-3, 0.1, k["rm"], k["rv"])
    R.check_box(dev, fn, ref[:c], d[:c], ref[c:], d[c:])
    mean = st[:c] / n
    var = (st[c:] / n - mean * mean).clamp_min(0)
    dev["running_var"] = 0.9 * k["rv"] + 0.1 * var
    with pytest.raises(AssertionError, match="running_var outside its box"):
        R.check_box(dev, fn, ref[:c], d[:c], ref[c:], d[c:])


def test_defect_8_d_with_the_wrong_sign_of_b_mean():
    k, c, n, _, _ = _finalize_inputs()
    g0 = torch.Generator().manual_seed(8)
    mean, invstd = torch.randn(c, generator=g0) * 0.3 + 0.3, torch.rand(c, generator=g0) + 0.5
    g, gerr = R.ref_g(k["dy"], 0)
    ref, mag, _ = R.ref_bwd_sums(g, gerr, k["x"])
    d = R.chain_rows(R.row_plan_bf16(n, c), R.fold_finalize) * R.U32 * mag
    st = ref.float()

    def fn(s0, s1):
        out = R.bwd_finalize_local(s0, s1, mean, invstd)
        out.update(R.bwd_finalize_global(s0, s1, n, k["gamma"], mean, invstd))
        return out
    dev = R.emu_bwd_finalize(st[:c], st[c:], st[:c], st[c:], n, k["gamma"], mean, invstd)
    R.check_box(dev, fn, ref[:c], d[:c], ref[c:], d[c:])
    dev["d"] = -(dev["a"] * st[:c]) / n + dev["b"] * mean
    with pytest.raises(AssertionError, match="d outside its box"):
        R.check_box(dev, fn, ref[:c], d[:c], ref[c:], d[c:])


# ---- the mirrors and the case tables --------------------------------------------------------------------------------------------------------
def test_row_plan_at_the_reduce_cap():
    plan = R.row_plan_bf16(32769, 1024)
    assert (plan.nblocks, plan.rows_per_block, plan.empty) == (2048, 17, 120)
    assert R.row_plan_bf16(32768, 1024).empty == 0
    assert all(R.row_plan_bf16(n, c).nblocks == 2048 and R.row_plan_bf16(n, c).empty > 0 for c, n in R.ROW["reduce_cap"])
    assert R.red_plan(*reversed(R.BN1D["reduce_cap"])).nblocks == 1024 and R.red_plan(*reversed(R.BN1D["reduce_cap"])).empty > 0


def test_row_launch_hits_its_cap():
    assert R.row_launch(131073, 1024) == R.RowLaunch(16384, 256, 2, 2)
    assert R.row_launch(131072, 1024).trips == 1
    c, n = R.ROW["apply_cap"]
    assert R.row_launch(n, c).trips == 2
    assert all(R.row_launch(n, c).trips == 1 for c, n in R.ROW["cases"])          # below the cap every thread makes exactly one trip
    assert R.row_launch(5, 24).threads == 255                                       # a group count that does not divide 256: one idle thread
    c, n = R.BN1D["apply_cap"]
    assert R.bn_apply_trips(n, c) == 2 and R.bn_apply_trips(n - 1, c) == 1
    assert R.cm_apply_trips(R.CM["apply_cap"][2]) == 2


def test_prefold_engages_exactly_above_1536_rows_and_up_to_128_channels():
    for nblocks in (1, 1535, 1536, 1537, 70000):
        for c in (16, 24, 128, 129, 136):
            assert R.partials_plan(nblocks, c).prefold == (nblocks > 1536 and 2 * c <= 256), (nblocks, c)
            assert not R.partials_plan(nblocks, c, with_ws=False).prefold
    p = R.partials_plan(4500, 16)
    assert (p.rows_per_slice, p.slices, p.ws_bytes) == (9, 500, 512 * 32 * 4)


def test_cm_plan_edges():
    assert R.cm_plan(2, 16, 4100).chunks == 2 and R.cm_plan(2, 16, 4100).chunk4 == 513
    b, c, pos = R.CM["chunks_by_channels"]
    assert R.cm_plan(b, c, pos).chunks == 64 < R.ceil_div(pos // 4, 1024)


def test_ulps():
    v = torch.tensor([0.0, 1.0, 1.5, 2.0, 255.0, 2.0 ** -130], dtype=torch.float64)
    assert R.ulp_fp32(v).tolist() == [2.0 ** -149, 2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -16, 2.0 ** -149]
    assert R.ulp_bf16(v).tolist() == [2.0 ** -133, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0 ** -133]


def test_every_batch_norm_entry_is_in_a_case_table():
    from sparse2dense_amd import _lib
    entries = {name for name in _lib.SIGNATURES if name.startswith(R.PREFIXES)}
    assert entries == R.table_entries(), (sorted(entries - R.table_entries()), sorted(R.table_entries() - entries))
    # the GPU file calls entries through R.entry alone, which refuses a name that is in no table and records what it hands out:
    # test_every_entry_of_the_case_tables_was_called there holds the record equal to the tables.  Here, only that each name is written out
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_bn_passes_gpu.py")).read()
    missing = sorted(name for name in entries if f'"{name}"' not in src)
    assert not missing, missing
    with pytest.raises(AssertionError, match="not in a case table"):
        R.entry(None, "s2d_lnwide_fwd")


def test_s2d_row_rpt_in_the_environment_is_refused():
    """in a child process: the import must fail with its message, and this process's module keeps its state"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, S2D_ROW_RPT="16")
    run = subprocess.run([sys.executable, "-c", "import bn_pass_ref"], cwd=here, env=env, capture_output=True, text=True)
    assert run.returncode != 0 and "S2D_ROW_RPT is set" in run.stderr, (run.returncode, run.stderr[-400:])
