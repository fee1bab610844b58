"""CPU-side checks of the drop-in boundary: libs2d_hip.so loads without a GPU and exports every
symbol include/s2d.h declares; argument validation returns error codes (no compute)."""
import ctypes
import os
import re

import pytest

from sparse2dense_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def declared_symbols(headers=("s2d.h", "s2d_debug.h")):
    """entry points of the boundary header and of the debug header (tools only: include/s2d_debug.h)"""
    names = set()
    for h in headers:
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(s2d_[a-z0-9_]+)\s*\(", src))
    return sorted(names)


def test_header_symbols_all_exported(lib):
    names = declared_symbols()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/s2d.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), "python binding and header disagree"
    assert not [n for n in declared_symbols(("s2d.h",)) if n.startswith("s2d_debug_")], "debug entries belong in include/s2d_debug.h"


def test_version_and_error_text(lib):
    assert lib.s2d_version() >= 100
    # invalid argument -> negative code + message, no HIP call is made
    rc = lib.s2d_voxelize_run(None, -5, 5, _lib.f6([0, 0, 0, 1, 1, 1]), _lib.f3([.1, .1, .1]), 5, 10, None, None, None,
                              None, None, None, 0, None)
    assert rc == -1
    assert "n_points" in _lib.last_error()
    with pytest.raises(_lib.S2DError):
        _lib.check(rc, "voxelize")


def test_workspace_queries(lib):
    assert lib.s2d_voxelize_workspace_bytes(150000, 5, 150000) > 150000 * 4
    wb = lib.s2d_rulebook_workspace_bytes(1, _lib.i3((41, 1504, 1504)), 100000)
    cells = 41 * 1504 * 1504
    assert wb >= cells // 32 * 8 and wb < cells  # 1 bit + prefix per 32 cells, far below spconv's int32 grid
    assert lib.s2d_spconv_wgrad_workspace_bytes(50000, 27, 16, 16) >= 27 * 256 * 4
    assert lib.s2d_bn1d_workspace_bytes(1000, 16) > 0
    assert lib.s2d_bn1d_workspace_bytes(1000, 5) == 0   # unsupported channel count


def test_launch_plans_of_the_dense_conv_kernels(lib):
    """Host-side launch plans (no device work): the pixel-tile height of the 3x3 conv is picked per launch and sizes the
    BN-statistics slabs; the weight-gradient kernel never launches more workgroups than CUs (256 assumed without a GPU)."""
    import torch
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("plan constants below are for 256 CUs")
    tiles = lib.s2d_conv2d3x3_stats_tiles
    m = 4 * 188 * 188
    assert tiles(4, 188, 188, 128, 128, 1, 1) == -(-m // 128)          # 1.44 rounds of resident workgroups: tall tiles
    assert tiles(4, 94, 94, 256, 256, 1, 1) == -(-(m // 4) // 96)       # below one round: 96-row tiles
    assert tiles(1, 188, 188, 128, 128, 1, 1) == -(-(m // 4) // 64)     # a quarter of a round: 64-row tiles
    assert tiles(4, 188, 188, 512, 64, 1, 1) == -(-m // 128)            # 64-wide column blocks: tap-shared kernel, 128 rows
    assert tiles(4, 190, 190, 128, 256, 0, 2) == -(-(4 * 94 * 94) // 96)
    assert tiles(4, 188, 188, 100, 128, 1, 1) == 0                       # unsupported channel count
    for shape, tiles_ in (((4, 188, 188, 128, 128, 1), 1), ((4, 94, 94, 256, 256, 1), 4), ((4, 188, 188, 512, 64, 1), 4)):
        splits = lib.s2d_conv2d3x3_wgrad_workspace_bytes(*shape) // (9 * shape[3] * shape[4] * 4)
        assert 0.9 * (256 // (3 * tiles_)) <= splits <= 256 // (3 * tiles_), (shape, splits)   # 3 kernel rows x tiles x splits <= 256
    assert lib.s2d_comm_ranks() == 0                                       # no communicator without a process group


def test_default_conv2d_plans_are_the_pinned_ones(lib):
    """With nothing forced, the plan report s2d_conv2d_plan (the function the launchers read) equals the launch arithmetic of the commit
    before the override entries existed, restated in tests/conv2d_ref.mirror_plan (conv_k32_rows cost model over 3 x CUs slots,
    conv_use_shared_a, conv1x1_use_k32), for the benchmark's layer shapes (tools/conv_bm_bench.py).  No launch."""
    import ctypes
    import torch
    import conv2d_ref as C
    for name in ("S2D_CONV_BM", "S2D_CONV_NS", "S2D_CONV_SHARED_A", "S2D_CONV1X1"):
        assert os.environ.get(name) is None, f"{name} is set: the library would not take its default plan"
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    assert lib.s2d_conv2d_debug_force(-1, -1, -1, -1) == 0
    shapes = [C.geo(C.K3, 4, 188, 188, 128, 128, 1, 1), C.geo(C.K3, 4, 188, 188, 64, 64, 1, 1), C.geo(C.K3, 4, 94, 94, 256, 256, 1, 1),
              C.geo(C.K3, 4, 188, 188, 512, 64, 1, 1), C.geo(C.K3, 4, 188, 188, 256, 128, 1, 1), C.geo(C.K3, 4, 188, 188, 128, 256, 1, 1),
              C.geo(C.K3, 4, 94, 94, 256, 512, 1, 1), C.geo(C.K3, 1, 188, 188, 128, 128, 1, 1), C.geo(C.K3, 4, 190, 190, 128, 256, 0, 2),
              C.geo(C.K3, 4, 188, 188, 128, 256, 1, 2), C.geo(C.K3_BNBWD, 4, 188, 188, 128, 128, 1, 1), C.geo(C.K3_BNBWD, 4, 94, 94, 256, 256, 1, 1),
              C.geo(C.K1, 4, 188, 188, 256, 256), C.geo(C.K1, 4, 188, 188, 256, 640), C.geo(C.K1, 4, 47, 47, 256, 1024),
              C.geo(C.K1, 4, 47, 47, 1024, 256), C.geo(C.K1, 4, 188, 188, 64, 64), C.geo(C.K1_BNBWD, 4, 47, 47, 1024, 256),
              C.geo(C.UP, 4, 47, 47, 256, 256, ks=4), C.geo(C.UP, 4, 94, 94, 256, 256, ks=4), C.geo(C.UP, 4, 94, 94, 256, 128, ks=3),
              C.geo(C.UP, 4, 58, 58, 64, 64, ks=4), C.geo(C.K4S2, 4, 94, 94, 256, 256), C.geo(C.K4S2, 4, 188, 188, 256, 256),
              C.geo(C.K2S2, 4, 376, 376, 64, 256), C.geo(C.K2S2, 4, 188, 188, 256, 256)]
    out = (ctypes.c_int32 * 8)()
    for g in shapes:
        assert lib.s2d_conv2d_plan(g.kind, g.n, g.h, g.w, g.cin, g.cout, g.pad, g.stride, g.ks, out) == 0, (g, _lib.last_error())
        assert C.Plan(*list(out)) == C.mirror_plan(g, cus), g
    if cus == 256:   # the values themselves, for the three tile heights of the cost model and the two other kernel families
        pinned = {0: (C.K32, 128, 128, 3, 1112, 1, 1, 1105), 2: (C.K32, 128, 96, 3, 376, 2, 1, 369), 3: (C.SHARED_A, 64, 128, 2, 1112, 1, 1, 1105),
                  7: (C.K32, 128, 64, 3, 560, 1, 1, 553), 16: (C.K64, 64, 128, 2, 1112, 1, 1, 1105), 18: (C.K32, 128, 96, 3, 96, 2, 4, 372)}
        for i, want in pinned.items():
            assert tuple(C.mirror_plan(shapes[i], 256)) == want, (shapes[i], C.mirror_plan(shapes[i], 256))


def test_default_conv2d_wgrad_plans_are_the_pinned_ones(lib):
    """With nothing forced, the plan report s2d_conv2d_wgrad_plan (the function the launchers and the three *_wgrad_workspace_bytes queries
    read) equals the launch arithmetic of the commit before the override entries existed, restated in tests/conv2d_wgrad_ref.mirror_plan
    (tiles of 128 where the channels allow, splits = CUs / (grid y * tiles) rounded down, clamped, re-derived from the rounded-up steps
    per workgroup; the deep ring), for the benchmark's 3x3, 1x1, 3x3 stride-2 and 4x4 stride-2 layer shapes.  No launch."""
    import ctypes
    import torch
    import conv2d_wgrad_ref as W
    assert os.environ.get("S2D_WG_RING_DEEP") is None, "S2D_WG_RING_DEEP is set: the library would not take its default plan"
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    assert lib.s2d_conv2d_wgrad_debug_force(-1, -1) == 0
    shapes = [W.geo(W.K3, 4, 188, 188, 128, 128, 1), W.geo(W.K3, 4, 94, 94, 256, 256, 1), W.geo(W.K3, 4, 188, 188, 512, 64, 1),
              W.geo(W.K3, 4, 188, 188, 64, 64, 1), W.geo(W.K3, 4, 188, 188, 256, 128, 1), W.geo(W.K3, 1, 188, 188, 128, 128, 1),
              W.geo(W.K1, 4, 188, 188, 256, 256), W.geo(W.K1, 4, 47, 47, 1024, 256), W.geo(W.K1, 4, 47, 47, 256, 1024), W.geo(W.K1, 4, 188, 188, 64, 64),
              W.geo(W.S2, 4, 188, 188, 128, 256, ks=3), W.geo(W.S2, 4, 376, 376, 64, 128, ks=3),
              W.geo(W.S2, 4, 94, 94, 256, 256, ks=4), W.geo(W.S2, 4, 188, 188, 256, 256, ks=4), W.geo(W.S2, 4, 116, 116, 64, 64, ks=4)]
    out = (ctypes.c_int32 * 8)()
    queries = {W.K3: lambda g: lib.s2d_conv2d3x3_wgrad_workspace_bytes.__wrapped__(g.n, g.h, g.w, g.cin, g.cout, g.pad),
               W.K1: lambda g: lib.s2d_conv2d1x1_wgrad_workspace_bytes.__wrapped__(g.n, g.h, g.w, g.cin, g.cout),
               W.S2: lambda g: lib.s2d_conv2d_s2_wgrad_workspace_bytes.__wrapped__(g.n, g.h, g.w, g.cout, g.cin, g.ks)}
    for g in shapes:
        assert lib.s2d_conv2d_wgrad_plan(g.kind, g.n, g.h, g.w, g.cin, g.cout, g.pad, g.ks, out) == 0, (g, _lib.last_error())
        plan = W.Plan(*list(out))
        assert plan == W.mirror_plan(g, cus), g
        assert plan.splits * plan.gy * plan.gz <= cus                      # never more workgroups than CUs
        assert queries[g.kind](g) == 4 * W.ws_floats(g, plan), g
    if cus == 256:   # the values themselves: 4512 K-steps on 85 -> 84 splits of 54; on 64 splits of 71; 376 on 8 splits of 47 (NS 5)
        pinned = {0: (128, 128, 8, 3, 84, 54, 3, 1), 6: (128, 128, 8, 1, 64, 71, 1, 4), 12: (128, 128, 5, 2, 8, 47, 8, 4)}
        for i, want in pinned.items():
            assert tuple(W.mirror_plan(shapes[i], 256)) == want, (shapes[i], W.mirror_plan(shapes[i], 256))
    # refused shapes: the report says so, the queries answer 0, a bad override changes nothing
    assert lib.s2d_conv2d_wgrad_plan(W.K3, 4, 188, 188, 100, 128, 1, 3, out) == -2 and lib.s2d_conv2d_wgrad_plan(W.S2, 4, 187, 188, 64, 64, 1, 3, out) == -2
    assert lib.s2d_conv2d_wgrad_debug_force(2, -1) == -1 and lib.s2d_conv2d_wgrad_debug_force(-1, 0) == -1
    assert lib.s2d_conv2d_wgrad_plan(W.K3, 4, 188, 188, 128, 128, 1, 3, out) == 0 and tuple(out) == tuple(W.mirror_plan(shapes[0], cus))
    try:   # the override reaches the report and the queries alike
        assert lib.s2d_conv2d_wgrad_debug_force(0, 7) == 0
        g = shapes[0]
        assert lib.s2d_conv2d_wgrad_plan(g.kind, g.n, g.h, g.w, g.cin, g.cout, g.pad, g.ks, out) == 0
        assert W.Plan(*list(out)) == W.mirror_plan(g, cus, deep=False, splits=7) and out[2] == 4 and out[4] == 7
        assert queries[g.kind](g) == 4 * W.ws_floats(g, W.Plan(*list(out)))
    finally:
        assert lib.s2d_conv2d_wgrad_debug_force(-1, -1) == 0


def test_ops_fail_loudly_on_cpu_tensors():
    import torch
    from sparse2dense_amd import hip_ops
    with pytest.raises(_lib.S2DError):
        hip_ops.voxelize(torch.zeros(10, 5), [.1, .1, .1], [0, 0, 0, 1, 1, 1], 5, 10)


def test_no_kernel_issues_mfmas_through_inline_asm():
    """DESIGN rule 31: an inline-asm MFMA is opaque to hipcc's hazard recognizer; the one kernel that used them (spconv_rg.hip, r03) computed wrong rows in its
    highest-pressure instantiation and left the tree."""
    import glob
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sparse2dense_amd", "csrc")
    hits = []
    for f in sorted(glob.glob(os.path.join(root, "*.hip")) + glob.glob(os.path.join(root, "*.h"))):
        for i, line in enumerate(open(f), 1):
            if re.search(r"asm[^;]*v_mfma", line):
                hits.append((os.path.basename(f), i))
    assert hits == []
