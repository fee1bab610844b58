"""heads.pooled_distill_loss through the fused kernels (csrc/pillar_distill.hip) against its float64 restatement on the host over the
same stored values, and one PointPillars distillation step (train_step.distill_loss) fused against S2D_PILLAR_DISTILL_FUSED=0.

Bounds: those of `masked_mse_pair` in tests/test_losses_gpu.py - value rtol 1e-5 (fp32 partial sums folded in double), gradient
1e-5 of its maximum for an fp32 student, 6e-3 of its maximum (one bf16 output rounding, 2^-8 = 3.9e-3) for a bf16 student."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sparse2dense_amd import heads

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
# (student dtype, student order, teacher dtype, teacher order): the four memory-order pairs; the first two are the tuned modes
BENCHMARKED = ("bf16", "cl", "f32", "nchw")
PARITY = ("f32", "nchw", "f32", "nchw")
COMBOS = [BENCHMARKED, PARITY, ("bf16", "cl", "bf16", "cl"), ("f32", "nchw", "bf16", "cl")]
# the strip kernel and the strided kernel with the other element types
EXTRA = [("f32", "cl", "bf16", "nchw"), ("bf16", "nchw", "f32", "cl")]
# one window and one channel group | odd both ways: a row and a column are dropped | 75 pooled pixels per row = two strips of 32 and
# a partial one, several blocks | more channels than the strip kernel's LDS tile takes: the strided kernel with a channels_last student
SHAPES = [(1, 8, 2, 2), (2, 64, 9, 13), (2, 64, 70, 150), (1, 200, 5, 6)]
FULL_ROW = (1, 8, 468, 468)   # the real row length
CASES = [(c, s) for c in COMBOS + EXTRA for s in SHAPES] + [(c, FULL_ROW) for c in (BENCHMARKED, PARITY)]

_CACHE = {}


def _order(t, order):
    return t.contiguous(memory_format=torch.channels_last) if order == "cl" else t.contiguous()


def _case(shape, sdt, tdt):
    """seeded inputs as stored in the maps' dtypes, and the float64 restatement over exactly those values (computed once per case)"""
    key = (shape, sdt, tdt)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(977 + sum(shape))
        student = lambda: (torch.round(torch.randn(shape, generator=g) * 4) / 4).to(DT[sdt])      # quarters: windows tie
        teacher = lambda: (torch.relu(torch.randn(shape, generator=g)) * (torch.rand(shape[0], 1, *shape[2:], generator=g) < 0.3)).to(DT[tdt])
        sa, sb, da, db = student(), student(), teacher(), teacher()
        if shape[2] * shape[3] < 16:   # a handful of cells: make sure both classes of both masks exist
            da[:, 0::2, 0, 0], db[:, 1::2, 0, 0] = 1.0, 1.0
            da[:, 1::2], db[:, 0::2] = 0.0, 0.0
        la, lb = sa.double().requires_grad_(True), sb.double().requires_grad_(True)
        ref = heads.pooled_distill_loss(la, da.double(), lb, db.double())
        ga, gb = torch.autograd.grad(ref, [la, lb])
        assert torch.isfinite(ref)
        _CACHE[key] = (sa, sb, da, db, float(ref.detach()), ga, gb)
    return _CACHE[key]


def _run(case, combo):
    sdt, so, tdt, to = combo
    sa, sb, da, db = case[:4]
    la, lb = (_order(t.to(DEV), so).requires_grad_(True) for t in (sa, sb))
    loss = heads.pooled_distill_loss(la, _order(da.to(DEV), to), lb, _order(db.to(DEV), to))
    ga, gb = torch.autograd.grad(loss, [la, lb])
    return loss.detach(), ga, gb, la, lb


def _check(got, want, bf16, what):
    tol = 6e-3 if bf16 else 1e-5
    err, top = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
    print(f"{what}: max err {err:.3e}, max {top:.3e}, ratio {err / top:.3e} (bound {tol:.0e})")
    assert err <= tol * top, what


@pytest.mark.parametrize("combo,shape", CASES, ids=lambda v: "-".join(str(x) for x in v))
def test_fused_matches_float64_restatement(combo, shape, monkeypatch):
    monkeypatch.delenv("S2D_PILLAR_DISTILL_FUSED", raising=False)
    case = _case(shape, combo[0], combo[2])
    ref, ra, rb = case[4:]
    loss, ga, gb, la, lb = _run(case, combo)
    print(f"loss {float(loss):.9g} vs {ref:.9g}, rel {abs(float(loss) - ref) / abs(ref):.3e}")
    np.testing.assert_allclose(float(loss), ref, rtol=1e-5)
    for g, leaf, r, name in ((ga, la, ra, "dF_S_a"), (gb, lb, rb, "dF_S_b")):
        assert g.dtype == leaf.dtype and g.stride() == leaf.stride() and g.shape == leaf.shape
        _check(g, r, combo[0] == "bf16", name)
        # routing: non-selected window elements and dropped rows / columns hold exactly 0 (a NaN there fails)
        assert bool((g.cpu()[r == 0] == 0).all()), name
    loss2, ga2, gb2, _, _ = _run(case, combo)
    assert torch.equal(loss, loss2) and torch.equal(ga, ga2) and torch.equal(gb, gb2)   # no atomics: bit-identical


def test_fused_path_is_taken(monkeypatch):
    """the default dispatch reaches the autograd function over the two entries (and S2D_PILLAR_DISTILL_FUSED=0 does not)"""
    case = _case(SHAPES[1], "bf16", "f32")
    monkeypatch.delenv("S2D_PILLAR_DISTILL_FUSED", raising=False)
    la = _order(case[0].to(DEV), "cl").requires_grad_(True)
    args = (la, case[2].to(DEV), _order(case[1].to(DEV), "cl"), case[3].to(DEV))
    assert "_PooledDistillFn" in type(heads.pooled_distill_loss(*args).grad_fn).__name__
    monkeypatch.setenv("S2D_PILLAR_DISTILL_FUSED", "0")
    assert "_PooledDistillFn" not in type(heads.pooled_distill_loss(*args).grad_fn).__name__


@pytest.mark.parametrize("combo,shape", [(c, SHAPES[2]) for c in COMBOS] + [(BENCHMARKED, FULL_ROW), (PARITY, FULL_ROW)],
                         ids=lambda v: "-".join(str(x) for x in v))
def test_fused_and_fallback_agree(combo, shape, monkeypatch):
    case = _case(shape, combo[0], combo[2])
    monkeypatch.delenv("S2D_PILLAR_DISTILL_FUSED", raising=False)
    loss, ga, gb, _, _ = _run(case, combo)
    monkeypatch.setenv("S2D_PILLAR_DISTILL_FUSED", "0")
    loss0, ga0, gb0, _, _ = _run(case, combo)
    np.testing.assert_allclose(float(loss), float(loss0), rtol=1e-5)
    for g, g0, name in ((ga, ga0, "dF_S_a"), (gb, gb0, "dF_S_b")):
        assert g.dtype == g0.dtype and g.stride() == g0.stride()
        _check(g, g0.double().cpu(), combo[0] == "bf16", name)
        assert bool((g[g0 == 0] == 0).all()), name


def test_unsupported_shapes_take_the_fallback_and_the_entry_refuses_them():
    from sparse2dense_amd import _lib
    from sparse2dense_amd.dense2d import _ptr, _ws
    lib = _lib.load()
    x = torch.randn(1, 12, 4, 4, device=DEV)   # c % 8 != 0
    t = torch.relu(torch.randn(1, 12, 4, 4, device=DEV))
    out = torch.empty(8, device=DEV)
    ws = _ws(lib.s2d_pooled_distill_workspace_bytes(), x.device)
    for c, h, w in ((12, 4, 4), (8, 1, 4), (8, 4, 1)):
        rc = lib.s2d_pooled_distill_fwd(x.data_ptr(), x.data_ptr(), 0, 0, t.data_ptr(), t.data_ptr(), 0, 0, 1, c, h, w, _ptr(out), _ptr(ws), ws.numel(), None)
        assert rc == -2 and "pooled_distill_fwd" in _lib.last_error()
    la = x.clone().requires_grad_(True)
    loss = heads.pooled_distill_loss(la, t, la * 0.5, t)
    assert "_PooledDistillFn" not in type(loss.grad_fn).__name__ and torch.isfinite(loss)


@pytest.fixture(scope="module")
def step_setup():
    from golden_util import fill_params
    from sparse2dense_amd import waymo_configs
    from sparse2dense_amd.data import SyntheticPillarFrames
    from sparse2dense_amd.registry import build_detector
    ex = SyntheticPillarFrames(1, n_points=12000, seed=31, distill=True, device=DEV).example()
    teacher = fill_params(build_detector(waymo_configs.centerpoint_pillar()), seed=1).to(DEV)
    student = fill_params(build_detector(waymo_configs.pillar_s2d_student()), seed=2).to(DEV).train()
    for p in teacher.parameters():
        p.requires_grad = False
    return ex, teacher, student


def _step(setup, fused, monkeypatch):
    """one distillation step on the shared models (no optimizer step in between; a train-mode batch norm does not read the running
    statistics the first call moved)"""
    from sparse2dense_amd.train_step import backward_and_clip, distill_loss
    ex, teacher, student = setup
    if fused:
        monkeypatch.delenv("S2D_PILLAR_DISTILL_FUSED", raising=False)
    else:
        monkeypatch.setenv("S2D_PILLAR_DISTILL_FUSED", "0")
    total, losses = distill_loss(teacher, student, ex)
    params = [p for p in student.parameters() if p.requires_grad]
    norm = backward_and_clip(total, params)
    return (float(total.detach()), {k: float(v[0]) for k, v in losses.items() if k != "loss" and torch.is_tensor(v[0]) and v[0].numel() == 1},
            {n for n, p in student.named_parameters() if p.grad is not None}, float(norm), losses)


def test_pillar_distillation_step_fused_vs_fallback(step_setup, monkeypatch):
    """wiring only (the arithmetic is pinned above): fp32 mode, CenterPoint-pillar teacher, S2D pillar student"""
    total1, terms1, with_grad1, norm1, losses = _step(step_setup, True, monkeypatch)
    total0, terms0, with_grad0, norm0, _ = _step(step_setup, False, monkeypatch)
    assert {"sparse2dense_loss", "kd_hm_loss", "T_hm_loss", "mask_loss", "reconstruction_loss"} <= set(terms1) and "kd_reg_loss" not in losses
    assert all(losses[k][0].is_cuda and not losses[k][0].requires_grad for k in ("sparse2dense_loss", "kd_hm_loss", "T_hm_loss"))
    assert np.isfinite(total1) and np.isfinite(norm1)
    print("terms fused", terms1, "\nterms fallback", terms0, "\ntotals", total1, total0, "norms", norm1, norm0)
    assert set(terms1) == set(terms0)
    for k in terms1:
        np.testing.assert_allclose(terms1[k], terms0[k], rtol=1e-5, err_msg=k)
    np.testing.assert_allclose(total1, total0, rtol=1e-5)
    assert with_grad1 == with_grad0 and with_grad1
    np.testing.assert_allclose(norm1, norm0, rtol=1e-4)
