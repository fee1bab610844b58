#!/usr/bin/env python
"""Generates tests/golden/pillar_distill.npz: the PointPillars branch of the reference's `TS_Trainer.batch_processor_inline`
(det3d/torchie/trainer/trainer.py:741-773) evaluated on seeded float64 inputs.

The statements of the branch are not restated here: the `if T_model.backbone._get_name() == "PointPillarsScatter":` body is cut out of
the reference's syntax tree (as make_golden.py does for `fastfocalloss`) and executed with stand-in models that return the seeded
tensors.  Only inputs and results are stored.

    python tests/golden/make_golden_pillar_distill.py          (reference at $S2D_REFERENCE, default /root/reference)

Inputs: feature maps 2 x 8 x 7 x 10 (odd height: the last row is dropped by the floor-mode pool), student values quantised to
quarters so that pooling windows tie, teacher maps relu(randn) under a 30 % cell mask so that both classes of both masks are
non-empty, a 3-class 12 x 16 heat map with five objects per frame."""
import ast
import os

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("S2D_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pillar_distill.npz")


def _functions(path, names):
    tree = ast.parse(open(os.path.join(REF, path)).read())
    return [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]


def _pillar_branch():
    """the statements under `if T_model.backbone._get_name() == "PointPillarsScatter":` of TS_Trainer.batch_processor_inline"""
    tree = ast.parse(open(os.path.join(REF, "det3d/torchie/trainer/trainer.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TS_Trainer"][0]
    fn = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "batch_processor_inline"][0]
    hits = [n for n in ast.walk(fn) if isinstance(n, ast.If) and isinstance(n.test, ast.Compare)
            and any(isinstance(c, ast.Constant) and c.value == "PointPillarsScatter" for c in n.test.comparators)]
    assert len(hits) == 1
    return hits[0].body


def tied_windows(x):
    """number of 2x2 windows (floor mode) whose maximum is attained more than once"""
    n, c, h, w = x.shape
    win = x[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    return int(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).sum())


def inputs():
    g = torch.Generator().manual_seed(20250117)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    shape = (2, 8, 7, 10)
    student = lambda: torch.round(rn(*shape) * 4) / 4
    teacher = lambda: torch.relu(rn(*shape)) * (torch.rand(shape[0], 1, *shape[2:], generator=g, dtype=torch.float64) < 0.3)
    a = dict(F_S_a=student(), F_S_b=student(), F_D_a=teacher(), F_D_b=teacher())
    hw = (12, 16)
    a["S_hm"] = torch.sigmoid(rn(2, 3, *hw)).clamp(1e-4, 1 - 1e-4)
    a["T_hm"] = rn(2, 3, *hw)
    a["hm"] = torch.rand(2, 3, *hw, generator=g, dtype=torch.float64) ** 4
    a["ind"] = torch.stack([torch.randperm(hw[0] * hw[1], generator=g)[:8] for _ in range(2)])
    a["cat"] = torch.randint(0, 3, (2, 8), generator=g)
    a["mask"] = torch.zeros(2, 8, dtype=torch.uint8)
    a["mask"][:, :5] = 1
    a["mask_loss"], a["offset_loss"], a["base_loss"] = (torch.tensor(v, dtype=torch.float64) for v in (0.8125, 0.34375, 1.5))
    return a


def main():
    a = inputs()
    assert tied_windows(a["F_S_a"]) >= 20 and tied_windows(a["F_S_b"]) >= 20
    for k in ("F_D_a", "F_D_b"):
        m = F.max_pool2d(a[k], 2, 2) > 0
        assert 0 < int(m.sum()) < m.numel()
    ns = {"torch": torch, "F": F}
    exec(compile(ast.Module(body=_functions("det3d/core/utils/center_utils.py", ("_gather_feat", "_transpose_and_gather_feat")),
                            type_ignores=[]), "center_utils_helpers", "exec"), ns)
    exec(compile(ast.Module(body=_functions("det3d/torchie/trainer/trainer.py", ("fastfocalloss",)), type_ignores=[]), "trainer_helpers", "exec"), ns)
    leaves = {k: a[k].clone().requires_grad_(True) for k in ("F_S_a", "F_S_b", "S_hm")}
    base = a["base_loss"].clone()
    ns["example"] = {k: [a[k]] for k in ("hm", "ind", "mask", "cat")}
    ns["T_model"] = lambda example, return_loss: ([{"hm": a["T_hm"]}], a["F_D_a"], a["F_D_b"])
    ns["S_model"] = lambda example, return_loss: ({"loss": [base * leaves["S_hm"].new_ones(())]}, leaves["F_S_a"], leaves["F_S_b"],
                                                  [{"hm": leaves["S_hm"]}], a["mask_loss"], a["offset_loss"])
    exec(compile(ast.Module(body=_pillar_branch(), type_ignores=[]), "pillar_branch", "exec"), ns)
    losses = ns["losses"]
    total = losses["loss"][0]
    grads = torch.autograd.grad(total, [leaves["F_S_a"], leaves["F_S_b"], leaves["S_hm"]])
    out = {k: v.numpy() for k, v in a.items()}
    keys = sorted(k for k in losses if k != "loss")
    out["log_keys"] = np.array(keys)
    for k in keys:
        out["log:" + k] = losses[k][0].detach().numpy()
    out["loss_increment"] = (total.detach() - a["base_loss"]).numpy()
    out["g:F_S_a"], out["g:F_S_b"], out["g:S_hm"] = (t.numpy() for t in grads)
    out["tied_windows"] = np.array([tied_windows(a["F_S_a"]), tied_windows(a["F_S_b"])])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: float(out["log:" + k]) for k in keys}, "increment", float(out["loss_increment"]),
          "tied", out["tied_windows"])


if __name__ == "__main__":
    main()
