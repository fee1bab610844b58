"""The workspace harness (tests/ws_guard.py) must be able to fail, and every workspace query must be accounted for.

The "entries" here are plain torch ops on CPU tensors inside allocations the harness owns: nothing touches a GPU or goes outside an
allocation.  The seams themselves are the product's (`nms._ws` & co. take a device), so the patching is exercised as the GPU tests
use it."""
import glob
import os
import re

import pytest
import torch

import ws_guard
from ws_guard import POISONS, GuardViolation, guard

CPU = torch.device("cpu")


def _request(nbytes=64):
    from sparse2dense_amd import nms
    return nms._ws(nbytes, CPU)


def _good_entry(ws):
    f = ws.view(torch.float32)
    f.copy_(torch.arange(f.numel(), dtype=torch.float32))   # writes every word ...
    return f.sum()                                          # ... before it reads any


def _reads_unwritten_entry(ws):
    return ws.view(torch.float32)[0].clone()


@pytest.mark.parametrize("poison", POISONS)
def test_well_behaved_entry_passes(monkeypatch, poison):
    from sparse2dense_amd import nms
    real = nms._ws
    with guard(monkeypatch, poison) as log:
        ws = _request(64)
        assert ws.numel() == 64 and ws.dtype == torch.uint8 and ws.data_ptr() % 256 == 0
        assert bool((ws == poison).all())
        out = _good_entry(ws)
    assert out.item() == sum(range(16))
    assert log.requests == [("nms", 64)]
    assert nms._ws is real   # the seam is restored


@pytest.mark.parametrize("poison", POISONS)
def test_write_one_byte_past_the_slice_trips_the_back_guard(monkeypatch, poison):
    with pytest.raises(GuardViolation, match=r"nms: the back guard of a 64-byte workspace .* byte 0 past the end"):
        with guard(monkeypatch, poison):
            ws = _request(64)
            _good_entry(ws)
            ws._base[ws.storage_offset() + ws.numel()] = 0
    from sparse2dense_amd import nms
    assert nms._ws.__name__ == "_ws"   # restored after a failure too


@pytest.mark.parametrize("poison", POISONS)
def test_write_one_byte_in_front_of_the_slice_trips_the_front_guard(monkeypatch, poison):
    with pytest.raises(GuardViolation, match=r"nms: the front guard of a 64-byte workspace .* 1 bytes in front"):
        with guard(monkeypatch, poison):
            ws = _request(64)
            _good_entry(ws)
            ws._base[ws.storage_offset() - 1] = 0


def test_a_strided_overrun_of_one_whole_request_is_still_inside_the_back_guard(monkeypatch):
    with pytest.raises(GuardViolation, match="back guard of a 8192-byte workspace"):
        with guard(monkeypatch, 0x5A):
            ws = _request(8192)
            ws._base[ws.storage_offset() + 2 * ws.numel() - 1] = 0   # the last byte of "one partial row too many"


def test_read_of_an_unwritten_word_differs_between_the_poisons(monkeypatch):
    got = []
    for poison in POISONS:
        with guard(monkeypatch, poison):
            got.append(_reads_unwritten_entry(_request(64)))
    assert torch.isnan(got[0]) and torch.isfinite(got[1]) and got[1].item() > 1e16   # 0xFF: NaN; 0x5A: ~1.5e16
    assert not torch.equal(got[0], got[1])
    assert got[1].view(torch.int32).item() == 0x5A5A5A5A and got[0].view(torch.int32).item() == -1


def test_floors_follow_the_real_helpers(monkeypatch):
    from sparse2dense_amd import anchors, dense2d, dense3d, hip_ops, nms, prep, solver
    with guard(monkeypatch, 0xFF) as log:
        sizes = [m._ws(8, CPU).numel() for m in (dense2d, dense3d, hip_ops)] + [hip_ops._ws_shared(8, CPU).numel()]
        sizes += [m._ws(8, CPU).numel() for m in (nms, anchors, prep, solver)]
        assert nms._ws(0, CPU).numel() == 0
    assert sizes == [256, 256, 256, 256, 8, 8, 8, 8]
    assert [m for m, _ in log.requests] == ["dense2d", "dense3d", "hip_ops", "hip_ops", "nms", "anchors", "prep", "solver", "nms"]
    # what the real exact-size helpers return for the same request
    assert hip_ops._ws(8, CPU).numel() == 256 and dense3d._ws(8, CPU).numel() == 256
    assert [m._ws(8, CPU).numel() for m in (nms, anchors, prep, solver)] == [8, 8, 8, 8]


def test_zero_is_no_poison(monkeypatch):
    with pytest.raises(AssertionError, match="zero hides"):
        with guard(monkeypatch, 0):
            pass


def test_every_workspace_site_of_the_package_goes_through_a_seam():
    """each module that defines a `_ws` / `_ws_shared` helper is patched by the harness, and no module but _debug.py sizes a torch.empty
    by a workspace query directly"""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sparse2dense_amd")
    found = set()
    for path in sorted(glob.glob(os.path.join(pkg, "*.py"))):
        name = os.path.splitext(os.path.basename(path))[0]
        src = open(path).read()
        found |= {(name, m) for m in re.findall(r"^def (_ws(?:_shared)?)\(", src, re.M)}
        if name != "_debug":
            direct = [ln for ln in src.splitlines() if re.search(r"torch\.empty\(.*_workspace_(bytes|floats)", ln)]
            assert not direct, (name, direct)
    assert found == {(m, a) for m, a, _ in ws_guard.SEAMS}


# ---- accounting: every workspace query of the C ABI is exercised under the harness, or exempt with a reason ---------------------------
_GPU = "tests.test_workspace_discipline_gpu::"
COVERED = {
    "s2d_conv2d3x3_wgrad_workspace_bytes": _GPU + "test_conv3x3_wgrad",
    "s2d_conv2d1x1_wgrad_workspace_bytes": _GPU + "test_conv1x1_wgrad",
    "s2d_conv2d_s2_wgrad_workspace_bytes": _GPU + "test_stride2_wgrad",
    "s2d_smallconv3x3_wgrad_workspace_bytes": _GPU + "test_small_cout_conv3x3",
    "s2d_dwconv7_wgrad_workspace_bytes": _GPU + "test_depthwise7",
    "s2d_bnrow_workspace_bytes": _GPU + "test_batchnorm2d_rows",
    "s2d_bn_partials_sum_workspace_bytes": _GPU + "test_partial_fold",
    "s2d_bn1d_workspace_bytes": _GPU + "test_bn1d",
    "s2d_lnwide_workspace_bytes": _GPU + "test_wide_layernorm",
    "s2d_bncm_workspace_bytes": _GPU + "test_bn3d_channel_major",
    "s2d_pointwise_conv_wgrad_workspace_bytes": _GPU + "test_pointwise_conv3d_wgrad",
    "s2d_convt3d_mfma_wgrad_workspace_bytes": _GPU + "test_convt3d_mfma_wgrad",
    "s2d_convt3d_k4s2p1_wgrad_workspace_bytes": _GPU + "test_convt3d_f32_wgrad",
    "s2d_spconv_wgrad_workspace_bytes": _GPU + "test_sparse_conv_wgrad",
    "s2d_rows_wgrad_workspace_bytes": _GPU + "test_pillar_rows_wgrad",
    "s2d_focal_workspace_bytes": _GPU + "test_focal",
    "s2d_center_tasks_loss_workspace_bytes": _GPU + "test_center_tasks_loss",
    "s2d_masked_mse_workspace_bytes": _GPU + "test_masked_mse",
    "s2d_pooled_distill_workspace_bytes": _GPU + "test_pooled_distill",
    "s2d_pcr_loss_workspace_bytes": _GPU + "test_pcr_loss",
    "s2d_pcr_heads_workspace_bytes": _GPU + "test_pcr_heads",
    "s2d_pcr_level_workspace_bytes": _GPU + "test_pcr_level",
    "s2d_anchor_assign_workspace_bytes": _GPU + "test_anchor_assign_and_loss",
    "s2d_anchor_loss_workspace_bytes": _GPU + "test_anchor_assign_and_loss",
    "s2d_nms_workspace_bytes": _GPU + "test_nms",
    "s2d_nms_batched_workspace_bytes": _GPU + "test_nms_batched",
    "s2d_deform_conv_bwd_data_workspace_bytes": _GPU + "test_deform_conv_backward",
    "s2d_deform_conv_wgrad_workspace_bytes": _GPU + "test_deform_conv_backward",
    "s2d_prep_workspace_bytes": _GPU + "test_compose_clouds",
    "s2d_voxelize_workspace_bytes": _GPU + "test_voxelize",
    "s2d_voxelize_batch_workspace_bytes": _GPU + "test_voxelize_batch",
    "s2d_rulebook_workspace_bytes": _GPU + "test_rulebook",
    "s2d_rulebook_chain_workspace_bytes": _GPU + "test_rulebook_chain",
    "s2d_rulebook_sort_workspace_bytes": _GPU + "test_rulebook_sort",
    "s2d_grad_norm_workspace_floats": _GPU + "test_grad_norm_and_clip",
}
# at most 4, each either without a caller outside _debug.py or reachable only with more than one GPU
EXEMPT = {
    "s2d_deform_conv_workspace_bytes": "no caller outside the tests: the forward entry takes no workspace and the query returns 0 (the sampled columns never leave LDS)",
}


def test_every_workspace_query_is_covered_or_exempt():
    from sparse2dense_amd import _lib
    names = {n for n in _lib.SIGNATURES if n.endswith(("_workspace_bytes", "_workspace_floats"))}
    assert len(names) >= 36
    assert not set(COVERED) & set(EXEMPT)
    assert set(COVERED) | set(EXEMPT) == names, (sorted(names - set(COVERED) - set(EXEMPT)), sorted((set(COVERED) | set(EXEMPT)) - names))
    assert len(EXEMPT) <= 4 and all(reason for reason in EXEMPT.values())
    import test_workspace_discipline_gpu as G
    for name, test_id in COVERED.items():
        fn = getattr(G, test_id.split("::")[1], None)
        assert callable(fn), test_id
        assert name in G.QUERIES[fn.__name__], (name, test_id)   # the test names the queries whose users it runs


def test_exempt_queries_have_no_caller_in_the_package():
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sparse2dense_amd")
    for name in EXEMPT:
        for path in glob.glob(os.path.join(pkg, "*.py")):
            if os.path.basename(path) in ("_lib.py", "_debug.py"):
                continue
            assert name + "(" not in open(path).read(), (name, path)
