"""Every entry of csrc/convt3d_mfma.hip against float64, at the shapes where its dispatch table branches.

The twelve entries (s2d_convt3d_mfma_fwd, _fwd_stats, _fwd_stats_y16, _fwd_stats_y16_norm, _fwd_stats_y16_norm_x16, _dgrad, _dgrad_d16,
_dgrad_d16_x16, _wgrad, _wgrad_d16, _wgrad_d16_norm, _wgrad_d16_norm_x16) are called through the C ABI (tests/convt3d_run.py); the test owns
every buffer: outputs, statistics rows, dW and the weight-gradient scratch are exact-size ws_guard allocations, poisoned (0xFF = NaN) and
fenced by guards that are checked after a synchronise.  tests/convt3d_ref.py states the operand model, the inputs, the bars and the shapes
(one comment per shape: the branch it reaches); tests/test_convt3d_variants_checks_cpu.py shows on the host that the checks reject the
defects they are there for.

Per shape and group (forward / data gradient / weight gradient):
  * every entry whose `*_supported` predicate accepts the shape runs and meets its float64 bar (fp32-stored: 1e-4 of max; bf16-stored:
    2^-8 |ref| + 1e-4 max elementwise); every entry whose predicate rejects it returns S2D_ERR_UNSUPPORTED and leaves its outputs poisoned;
  * the epilogue statistics fold (float64, on the host) to the sums over the STORED output, every partial row finite;
  * the bit identities the kernels' comments promise: y16 == bf16(y32); a _d16 form fed bf16(dout) == the fp32 form fed the widened values;
    an _x16 form == the fp32-x form; din of _dgrad_d16_x16 == bf16(din of _dgrad_d16); a _norm form == the plain form fed the tensor
    normalised on the host (exact by the choice of inputs);
  * weight gradients run under both scratch poisons and give equal bits.
Three shapes run again with unrounded fp32 x, w and dout (the forms without the fold): the reference rounds with torch, and the fp32-dout
form must equal the _d16 form fed torch's rounding bit for bit - the loads round to nearest even.

Not reached: the staged data-gradient kernel (ct_dgrad_mfma_kernel) runs only when one sample's fp32 dout reaches 2 GB.
"""
import pytest
import torch

import convt3d_ref as R

pytestmark = pytest.mark.gpu

GROUPS = ("forward", "dgrad", "wgrad")
_DC = {}


def _device_case(key, rounded=True):
    """the device copy of a case; one shape resident at a time (the cases run shape-major)"""
    import convt3d_run as G
    if (key, rounded) not in _DC:
        _DC.clear()
        _DC[(key, rounded)] = G.DeviceCase(R.case(key, rounded))
    return _DC[(key, rounded)]


def _run_group(group, dc, rep):
    import convt3d_run as G
    {"forward": G.forward_case, "dgrad": G.dgrad_case, "wgrad": G.wgrad_case}[group](dc, rep)


def test_predicates_and_plans_match_the_host_restatement():
    """the `*_supported` predicates, the statistics row count and the weight-gradient scratch size are what tests/convt3d_ref.py expects of
    each shape - the branch facts asserted in test_convt3d_variants_checks_cpu.py are facts about THIS library"""
    from sparse2dense_amd import _lib
    lib = _lib.load()
    for key, cin, cout, shp in R.SHAPES:
        n, d, h, w = shp
        assert bool(lib.s2d_convt3d_mfma_supported(cin, cout)) == R.expect_mfma(cin, cout), key
        assert bool(lib.s2d_convt3d_mfma_d16_supported(cin, cout, d, h, w)) == R.expect_d16(cin, cout, shp), key
        assert bool(lib.s2d_convt3d_mfma_norm_supported(cin, cout, d, h, w)) == R.expect_norm(cin, cout, shp), key
        assert bool(lib.s2d_convt3d_mfma_x16_supported(cin, cout, d, h, w)) == R.expect_x16(cin, cout, shp), key
        assert lib.s2d_convt3d_mfma_wgrad_workspace_bytes(n, cin, cout, d, h, w) == R.wgrad_plan(cin, cout, shp)["ws_bytes"], key
        yr = 1 if cin == 32 else 4
        assert lib.s2d_convt3d_mfma_stats_tiles(n, cin, d, h, w) == n * (1 if cin == 16 else d) * (-(-h // yr)) * (-(-w // 64)), key


@pytest.mark.parametrize("key,group", [(k, g) for k, *_ in R.SHAPES for g in GROUPS], ids=lambda v: str(v))
def test_entries_against_float64(key, group):
    rep = R.Report()
    _run_group(group, _device_case(key), rep)
    rep.assert_all(f"{key} {group}")


@pytest.mark.parametrize("key,group", [(k, g) for k in R.UNROUNDED for g in GROUPS], ids=lambda v: str(v))
def test_unrounded_inputs_are_rounded_to_nearest_even_on_load(key, group):
    rep = R.Report()
    _run_group(group, _device_case(key, rounded=False), rep)
    rep.assert_all(f"{key} {group} unrounded")
