"""The checking code of tests/test_spconv_plans_gpu.py, run on the host against hand-made launch results: a right one passes, the r04
defect (the second tile of a wave holds wrong rows), a tile nobody stored and a store past the buffer are each rejected.  No library
call: the "kernel output" is the float64 reference rounded to bf16."""
import pytest
import torch

import test_spconv_plans_gpu as P

T = 11                      # <MI = 2, WAVES = 8> with 11 tiles per workgroup: waves 0..2 own a second tile (tile 8 + wave)
N_OUT = P.rows_for(T)
CIN, COUT, KVOL, N_IN = 16, 32, 27, 300


def _problem():
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(N_IN, CIN, generator=g).to(torch.bfloat16)
    w = torch.randn(KVOL, CIN, COUT, generator=g) * 0.1
    bias = torch.randn(COUT, generator=g)
    nbr = torch.randint(0, N_IN, (KVOL, N_OUT), dtype=torch.int32, generator=g)
    nbr[torch.rand(KVOL, N_OUT, generator=g) < 0.5] = -1
    return P._ref_conv(feat, w, bias, nbr, N_OUT)


def _launch_result(ref):
    """what a correct launch leaves in the poisoned buffers: (obuf, out, pbuf, partial), one statistics row per workgroup"""
    obuf, out = P.poisoned(N_OUT, COUT, dtype=torch.bfloat16, device="cpu")
    out.copy_(ref.to(torch.bfloat16))
    groups = P.ceil_div(P.ceil_div(N_OUT, 16), T)
    pbuf, partial = P.poisoned(groups, 2, COUT, dtype=torch.float32, device="cpu")
    for b in range(groups):
        rows = out[16 * T * b:16 * T * (b + 1)].float()
        partial[b, 0], partial[b, 1] = rows.sum(0), (rows * rows).sum(0)
    return obuf, out, pbuf, partial


def test_checks_accept_a_correct_launch():
    ref = _problem()
    obuf, out, pbuf, partial = _launch_result(ref)
    P.check_launch(obuf, pbuf)
    P.check_output(out, partial, ref, out.clone())


def test_checks_reject_a_wrong_second_tile_of_a_wave():
    """rows of wave 0's second tile (tile 8 of the first workgroup) replaced by its first tile's rows: written and finite, so only the
    comparisons can see it - each of them does"""
    ref = _problem()
    obuf, out, pbuf, partial = _launch_result(ref)
    good = out.clone()
    out[16 * 8:16 * 9] = good[0:16]
    P.check_launch(obuf, pbuf)
    with pytest.raises(AssertionError, match="rows off the reference"):
        P.assert_parity(out, ref)
    with pytest.raises(AssertionError, match="differ from the default plan"):
        P.assert_same_bits(out, good)
    with pytest.raises(AssertionError, match="stored rows"):
        P.assert_stats(out, partial)   # (the statistics rows were summed from the right accumulators)
    with pytest.raises(AssertionError):
        P.check_output(out, partial, ref, good)
    # one element off by one bf16 ulp: inside the parity tolerance, caught by the bit comparison alone
    out.copy_(good)
    bits = out.view(torch.int16)
    bits[200, 3] += 1
    P.assert_parity(out, ref)
    with pytest.raises(AssertionError, match="differ from the default plan"):
        P.assert_same_bits(out, good)


def test_checks_reject_a_tile_left_at_the_fill():
    ref = _problem()
    obuf, out, pbuf, partial = _launch_result(ref)
    out[16 * 9:16 * 10] = float("nan")   # a skipped tile keeps the poison
    with pytest.raises(AssertionError, match="rows left at the NaN fill"):
        P.check_launch(obuf, pbuf)
    with pytest.raises(AssertionError, match="rows off the reference"):
        P.assert_parity(out, ref)          # a NaN never passes as "close"
    obuf, out, pbuf, partial = _launch_result(ref)
    partial[1] = float("nan")              # a workgroup that stored no statistics row
    with pytest.raises(AssertionError, match="partial: rows left at the NaN fill"):
        P.check_launch(obuf, pbuf)


@pytest.mark.parametrize("where", ["front", "back"])
def test_checks_reject_a_store_outside_the_buffer(where):
    ref = _problem()
    obuf, out, pbuf, partial = _launch_result(ref)
    obuf[P.GUARD - 1 if where == "front" else -P.GUARD, 0] = 0.0
    with pytest.raises(AssertionError, match=f"out: {where} guard rows overwritten"):
        P.check_launch(obuf, pbuf)
    obuf, out, pbuf, partial = _launch_result(ref)
    # a NaN of another bit pattern is a store too
    pbuf.view(torch.int32)[0 if where == "front" else -1, 1, 2] ^= 1
    with pytest.raises(AssertionError, match=f"partial: {where} guard rows overwritten"):
        P.check_launch(obuf, pbuf)
