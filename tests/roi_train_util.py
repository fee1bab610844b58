"""Shared by test_roi_train_cpu.py and test_roi_train_gpu.py: heads, seeded cases, the fp32 torch "chain" of the RoI MLP's training branch
with caller-supplied dropout masks, the three ways to run one training step of the head (float64 definition, fp32 chain, kernels), and the
project's parity rule for them."""
import copy

import torch
from torch import nn

from golden_util import fill_params, seeded
from sparse2dense_amd import registry, second_stage as S

LOSS_CFG = dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="L1",
                LOSS_WEIGHTS={"rcnn_cls_weight": 1.0, "rcnn_reg_weight": 0.5, "code_weights": [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0]})

#          cin   shared      cls         reg         rows  seed
SHAPES = [(2560, (256, 256), (256, 256), (256, 256), 37, 0),   # the two-stage configs: ten staged chunks, three row tiles, the last one ragged
          (40, (64, 64), (), (64, 64), 17, 0),                 # CLS_FC = []: the cls final layer reads the shared activation; single k-steps
          (512, (256,), (256, 256), (256, 256), 16, 0)]        # one shared layer; exactly one row tile
TWO_ROWS = (40, (64,), (64,), (64,), 2, 0)                     # x_hat = +-1: forward, statistics, losses and the final layers' gradients only


def make_train_head(cin, shared, cls, reg, dp=0.3, seed=0, **cfg):
    """a RoIHead in training mode with test_roi_mlp_cpu.make_head(..., signed=True) weights: N(0, 1.5 / cin) convolutions, so that the sums
    cancel as a trained head's do"""
    cfg = dict(dict(CLASS_AGNOSTIC=True, SHARED_FC=list(shared), CLS_FC=list(cls), REG_FC=list(reg), DP_RATIO=dp, LOSS_CONFIG=LOSS_CFG), **cfg)
    head = registry.build(dict(type="RoIHead", input_channels=cin, code_size=7, model_cfg=cfg), registry.ROI_HEAD)
    fill_params(head, seed)
    with torch.no_grad():
        for i, m in enumerate(m for m in head.modules() if isinstance(m, nn.Conv1d)):
            m.weight.copy_(seeded(m.weight.shape, 1000 + 17 * seed + i, (1.5 / m.in_channels) ** 0.5))
    return head.train()


def draw_masks(head, rows, seed):
    """one 0/1 float mask [rows, width] per dropout site of the head, from a seeded CPU generator"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((rows, w), generator=g) >= p).float() for w, p in S.roi_mlp_train_sites(head)]


def make_case(cin, rows, seed):
    """features, soft labels with a few ignored (-1) rows, a foreground mask and 8-column targets (gt_of_rois carries the class behind
    the 7 residuals)"""
    g = torch.Generator().manual_seed(100 + seed)
    labels = torch.rand((rows,), generator=g)
    labels[torch.arange(rows) % 5 == 3] = -1.0
    fg = (torch.arange(rows) % 3 != 1).long()
    return dict(x=seeded((rows, cin), 11 + seed), labels=labels, fg=fg, target=seeded((rows, 8), 12 + seed, 0.5))


def chain_mlp(head, x, masks=None):
    """the three nn.Sequential's of `head` as RoIHead.forward runs them, every nn.Dropout replaced by `* mask / (1 - p)` (masks=None:
    by nothing): x [R, cin] -> (rcnn_cls [R, 1], rcnn_reg [R, 7]).  Moves the running statistics of a head in training mode."""
    site = [0]

    def run(seq, t):
        for m in seq:
            if isinstance(m, nn.Dropout):
                if masks is not None:
                    t = t * masks[site[0]].to(t).unsqueeze(-1) / (1 - m.p)
                site[0] += 1
            else:
                t = m(t)
        return t
    shared = run(head.shared_fc_layer, x.reshape(-1, 1, x.shape[-1]).permute(0, 2, 1).contiguous())
    return (run(head.cls_layers, shared).transpose(1, 2).contiguous().squeeze(dim=1), run(head.reg_layers, shared).transpose(1, 2).contiguous().squeeze(dim=1))


def head_cls_loss(head, ret):
    """RoIHead.get_box_cls_layer_loss on the rows it does not ignore: the same sum over the same rows, divided by the same count.  Current
    torch refuses the ignored rows' label of -1 in binary_cross_entropy before the head can mask them out - with an error on the CPU and with
    a device-side assertion, which ends the process's GPU work, on the device - so the head's function never sees those rows here."""
    labels = ret["rcnn_cls_labels"].reshape(-1)
    keep = labels >= 0
    return head.get_box_cls_layer_loss(dict(rcnn_cls=ret["rcnn_cls"].reshape(-1, 1)[keep], rcnn_cls_labels=labels[keep]))[0]


def layers_of(head):
    """[(conv, bn | None)] in the order shared, cls, reg"""
    return [pair for seq in (head.shared_fc_layer, head.cls_layers, head.reg_layers) for pair in S._mlp_chain(seq)]


def run_step(head, case, masks, how):
    """One training step of a COPY of `head` on `case`: forward, both losses, backward of their sum.  how = "ref" (the float64 definitions),
    "chain" (fp32 torch modules with the same masks and the head's own loss functions) or "fused" (the kernels).  Returns
    dict(out [R, 8], loss_cls, loss_reg, layers=[dict(w, gamma, beta | bias: gradients; mean, var: running statistics)])."""
    dev = next(head.parameters()).device
    head = copy.deepcopy(head)
    x, labels, fg, target = (case[k].to(dev) for k in ("x", "labels", "fg", "target"))
    if how == "ref":
        head = head.double()
        cls, reg, stats = S.roi_mlp_train_reference(head, x.double(), masks)
        with torch.no_grad():
            for (_, bn), (mean, var) in zip([l for l in layers_of(head) if l[1] is not None], stats):
                bn.running_mean.mul_(1 - bn.momentum).add_(bn.momentum * mean)
                bn.running_var.mul_(1 - bn.momentum).add_(bn.momentum * var)
        loss_cls, loss_reg = S.roi_loss_reference(cls, reg, labels.double(), fg, target.double(), LOSS_CFG)
    elif how == "chain":
        cls, reg = chain_mlp(head, x, masks)
        ret = dict(rcnn_cls=cls, rcnn_reg=reg, rcnn_cls_labels=labels, reg_valid_mask=fg, gt_of_rois=target)
        loss_cls, loss_reg = head_cls_loss(head, ret), head.get_box_reg_layer_loss(ret)[0]
    else:
        cls, reg = S.roi_mlp_train_fused(head, x, masks)
        loss_cls, loss_reg = S.roi_loss_fused(cls, reg, labels, fg, target, LOSS_CFG)
    (loss_cls + loss_reg).backward()
    return collect(head, cls, reg, loss_cls, loss_reg)


def collect(head, cls, reg, loss_cls, loss_reg):
    """what `check_step` compares, from a head behind its backward"""
    layers = []
    for conv, bn in layers_of(head):
        if bn is None:
            layers.append(dict(w=conv.weight.grad, bias=conv.bias.grad))
        else:
            layers.append(dict(w=conv.weight.grad, gamma=bn.weight.grad, beta=bn.bias.grad, mean=bn.running_mean.detach(), var=bn.running_var.detach(),
                               tracked=int(bn.num_batches_tracked)))
    return dict(out=torch.cat([cls, reg], dim=1).detach(), loss_cls=loss_cls.detach(), loss_reg=loss_reg.detach(), layers=layers)


def errors(ref, got):
    """(max |got - ref|, max |ref|) in float64"""
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max()), float(ref.abs().max())


def check_pool(name, triples, fused=True):
    """The parity rule on a pool of (ref, chain, fused) tensors, each divided by its own max|ref|: with e the largest such relative error
    over the pool, e_fused <= 4 e_chain + 1e-7.  For a single tensor this is e_fused <= 4 e_chain + 1e-7 max|ref| as test_roi_mlp_gpu.py
    states it.  Conditions on the reference and the chain alone: every max|ref| finite and > 0, every e_chain < 1e-3 max|ref|.
    fused=False checks the conditions only (seed selection on the CPU, where no kernel runs)."""
    e_chain = e_fused = 0.0
    for ref, chain, got in triples:
        ec, top = errors(ref, chain)
        assert 0 < top < float("inf"), (name, top)
        assert ec < 1e-3 * top, (name, ec, top)
        e_chain = max(e_chain, ec / top)
        if fused:
            assert got.shape == ref.shape and got.dtype == torch.float32, (name, got.shape, got.dtype)
            e_fused = max(e_fused, errors(ref, got)[0] / top)
    print(f"{name}: e_chain {e_chain:.3e}, e_fused {e_fused:.3e} (relative to max|ref|)")
    if fused:
        assert e_fused <= 4 * e_chain + 1e-7, (name, e_fused, e_chain)


def check_step(ref, chain, got, data_grads=True, fused=True):
    """the rule on everything one step produces.  Pools: (rcnn_cls | rcnn_reg) with the two loss scalars, which have no layer of their own;
    per layer the weight gradient with that layer's tensors of fewer than 256 elements (gamma / beta gradients of a narrow layer, a final
    bias); a gamma or beta gradient of 256 elements on its own; per hidden layer the two running statistics.  data_grads=False (two rows)
    leaves out the gradients below the final layers."""
    got = got if fused else chain
    pick = lambda key, l=None: tuple((r if l is None else r["layers"][l])[key] for r in (ref, chain, got))
    check_pool("outputs and losses", [pick("out"), pick("loss_cls"), pick("loss_reg")], fused)
    for l, layer in enumerate(ref["layers"]):
        final = "bias" in layer
        if not final:
            check_pool(f"layer {l} running statistics", [pick("mean", l), pick("var", l)], fused)
            assert got["layers"][l]["tracked"] == chain["layers"][l]["tracked"]
        if not final and not data_grads:
            continue
        pool, small = [pick("w", l)], ("bias",) if final else ("gamma", "beta")
        for key in small:
            if layer[key].numel() < 256:
                pool.append(pick(key, l))
            else:
                check_pool(f"layer {l} d{key}", [pick(key, l)], fused)
        check_pool(f"layer {l} dW" + (" + " + ", ".join(small) if len(pool) > 1 else ""), pool, fused)
