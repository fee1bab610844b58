"""TEST INFRASTRUCTURE ONLY - the autograd contract of a layer with a hand-written backward, as checkers over a `Case`.

The kernel parity suites reach every torch.autograd.Function in one configuration: all leaves trainable, one dense upstream gradient, one
forward and one backward.  The Python between autograd and the kernels branches on exactly what they hold constant (ctx.needs_input_grad,
the layout of dy, caches keyed by parameter version, tags left on tensors).  The contracts below vary those and nothing else:

  (a) masks          every subset of the leaves as the trainable set: y and dx bit-stable, requested gradients within tolerance of float64,
                     frozen leaves keep .grad None; optionally again under other execution modes (side stream), bit-equal
  (b) grad_forms     the same upstream values handed over in other memory layouts: gradients bit-equal to the dense hand-over
  (c) replay         two backwards over one retained graph agree bit for bit; saved inputs, parameters and buffers keep their bits
  (d) interleave     fwd A, fwd B, bwd B, bwd A through one module equals the isolated runs; accumulate: .grad == gA + gB exactly
  (e) grad_mode      no_grad (and eval, for layers without statistics) forward is bit-equal to the grad-enabled one
  (f) param_update   linear layers: doubled parameters double y and dx exactly and leave dw alone; load_state_dict / a raw write +
                     refresh equals a freshly built module
  (g) fanout         x feeds the layer and an identity skip: x.grad == dx_alone + G_skip exactly
  (h) stale_tags     producer -> in-place op -> norm: the norm sees the modified tensor (and the tag IS consumed without the op)

Pure torch: runs on the CPU (tests/test_autograd_contract_checks_cpu.py shows on toy Functions with one seeded defect each that every
contract can fail) and on the GPU (tests/test_autograd_contract_gpu.py).  Never imports the product.

Reference: `Case.ref(ops)` is the stock layer's mathematics; the harness evaluates it in float64 on the CPU over the very operands the
device run held (already rounded to their storage types) and differentiates it with torch.autograd.
Tolerances: relative to max|ref| per tensor, supplied by the case from the layer's existing float64 test (or the 8e-3 bf16 / 2e-3 fp32
bounds derived in the header of tests/test_s16_gpu.py).  Most assertions are bit equalities and have none.  A gradient summed with float
atomics (`Case.inexact`) cannot be bit-stable: wherever a bit equality is asked of it, it is held to its tolerance against float64.
"""
import contextlib
import itertools

import torch


class ContractError(AssertionError):
    def __init__(self, case, contract, leaf, msg):
        self.case, self.contract, self.leaf = case, contract, leaf
        super().__init__(f"[{case}] contract ({contract}) leaf {leaf}: {msg}")


class Case:
    """One layer configuration.
    build(device) -> module          deterministic: seeds itself; parameters hold storage-representable values
    inputs(seed, device) -> dict     name -> tensor, storage-representable values; names in `leaves` are differentiable
    call(module, inputs) -> y        one tensor
    params(module) -> dict           leaf name ("weight", "bias" / "gamma", "beta") -> Parameter
    ref(ops) -> y                    stock mathematics over ops = {input and parameter names -> float64 CPU tensors}
    tol                              leaf name or "y" -> bound relative to max|ref|
    leaves                           names of the differentiable inputs ("x", "residual")
    context()                        context manager around every forward (autocast)
    scope()                          context manager around every forward AND every backward: a global mode that both passes read
    inexact                          leaf names whose gradient is summed with float atomics (exempt from bit equality)
    linear                           y is linear in (weight, bias) jointly and in x: contract (f) applies
    has_stats                        the forward depends on module.training (contract (e) skips the eval comparison)
    buffers(module) -> dict          state that a forward legitimately changes is NOT listed; what a BACKWARD must not change is
    grad_like(y, seed) -> G          upstream gradient; default: normal values rounded to y's dtype, in y's layout
    """

    def __init__(self, name, build, inputs, call, params, ref, tol, leaves=("x",), context=contextlib.nullcontext, inexact=(),
                 linear=False, has_stats=False, sync=None, grad_like=None, scope=contextlib.nullcontext):
        self.name, self.build, self.inputs, self.call, self.params, self.ref, self.tol = name, build, inputs, call, params, ref, tol
        self.leaves, self.context, self.inexact, self.linear, self.has_stats = tuple(leaves), context, frozenset(inexact), linear, has_stats
        self.sync = sync or (lambda: None)
        self.grad_like = grad_like or default_grad
        self.scope = scope


TALLY = {"bit": 0, "tol": 0, "max_ratio": 0.0}
RECORD = {}   # (case, contract) -> dict(bit=, tol=, max_ratio=)
_current = [None]


@contextlib.contextmanager
def _recording(case, contract):
    key = (case.name, contract)
    rec = RECORD.setdefault(key, {"bit": 0, "tol": 0, "max_ratio": 0.0, "status": "fail"})
    prev, _current[0] = _current[0], rec
    try:
        yield
        rec["status"] = "pass"
    finally:
        _current[0] = prev


def _count(kind, ratio=None):
    for rec in (TALLY, _current[0]):
        if rec is None:
            continue
        rec[kind] += 1
        if ratio is not None:
            rec["max_ratio"] = max(rec["max_ratio"], ratio)


def default_grad(y, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    vals = torch.randn(tuple(y.shape), generator=g).to(y.dtype)
    return torch.empty_like(y).copy_(vals.to(y.device))


def _first_diffs(a, b, k=4):
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape:
        return f"shapes {tuple(a.shape)} vs {tuple(b.shape)}"
    ne = (a != b) & ~(torch.isnan(a) & torch.isnan(b))
    idx = ne.nonzero()[:k]
    items = [f"{tuple(i.tolist())}: {a[tuple(i.tolist())].item()!r} vs {b[tuple(i.tolist())].item()!r}" for i in idx]
    return f"{int(ne.sum())} of {a.numel()} elements differ, first " + "; ".join(items)


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.detach().cpu(), b.detach().cpu())


def _require_bits(case, contract, leaf, a, b, what, ref=None):
    """a and b bit-equal; a leaf in case.inexact is held to its tolerance against the float64 `ref` instead (both sides)"""
    if leaf in case.inexact and ref is not None:
        _require_close(case, contract, leaf, a, ref, what)
        _require_close(case, contract, leaf, b, ref, what)
        return
    _count("bit")
    if (a is None) != (b is None):
        raise ContractError(case.name, contract, leaf, f"{what}: one side is None ({a is None} / {b is None})")
    if not bits_equal(a, b):
        raise ContractError(case.name, contract, leaf, f"{what}: not bit-identical: {_first_diffs(a, b)}")


def _require_close(case, contract, leaf, a, ref, what):
    tol = case.tol[leaf]
    if a is None:
        raise ContractError(case.name, contract, leaf, f"{what}: gradient is None")
    a64, r = a.detach().double().cpu(), ref.detach().double()
    if a64.shape != r.shape:
        raise ContractError(case.name, contract, leaf, f"{what}: shape {tuple(a64.shape)} vs reference {tuple(r.shape)}")
    scale = float(r.abs().max())
    err = float((a64 - r).abs().max()) if r.numel() else 0.0
    bound = tol * scale
    _count("tol", err / bound if bound > 0 else (0.0 if err == 0 else float("inf")))
    if not err <= bound:
        bad = ((a64 - r).abs() > bound).nonzero()[:4]
        items = [f"{tuple(i.tolist())}: {a64[tuple(i.tolist())].item()!r} vs {r[tuple(i.tolist())].item()!r}" for i in bad]
        raise ContractError(case.name, contract, leaf, f"{what}: |err| {err:.4g} > {tol:g} * max|ref| = {bound:.4g}; first " + "; ".join(items))


# ----------------------------------------------------------------------------------------------------------------------------------
class Run:
    """one forward (+ backward) of a case: y, the leaf tensors, their gradients"""

    def __init__(self, case, device, seed=0, mask=None, module=None, grad_mode=True):
        self.case = case
        self.module = case.build(device) if module is None else module
        self.inputs = case.inputs(seed, device)
        self.leaf = {k: self.inputs[k] for k in case.leaves}
        self.leaf.update(case.params(self.module))
        self.mask = set(self.leaf) if mask is None else set(mask)
        for k, t in self.leaf.items():
            t.requires_grad_(k in self.mask)
            t.grad = None
        with case.scope(), case.context(), (contextlib.nullcontext() if grad_mode else torch.no_grad()):
            self.y = case.call(self.module, self.inputs)

    def backward(self, G, retain=False):
        if self.y.requires_grad:
            with self.case.scope():
                self.y.backward(G, retain_graph=retain)
        self.case.sync()
        return self.grads()

    def grads(self):
        return {k: (None if t.grad is None else t.grad.detach().clone()) for k, t in self.leaf.items()}

    def reference(self, G):
        """float64 on the CPU over the operands this run held"""
        ops = {k: v.detach().double().cpu() for k, v in self.inputs.items() if torch.is_tensor(v)}
        ops.update({k: v.detach().double().cpu() for k, v in self.leaf.items()})
        for k in self.leaf:
            ops[k].requires_grad_(True)
        y = self.case.ref(ops)
        names = list(self.leaf)
        gs = torch.autograd.grad(y, [ops[k] for k in names], G.detach().double().cpu().reshape(y.shape), allow_unused=True)
        return y.detach(), {k: (torch.zeros_like(ops[k]) if g is None else g) for k, g in zip(names, gs)}


def _all_masks(names):
    names = list(names)
    for r in range(len(names), -1, -1):
        for sub in itertools.combinations(names, r):
            yield set(sub)


def contract_masks(case, device, modes=()):
    """(a).  modes: (label, context manager factory[, used]) alternatives (side stream on) under which every gradient must equal the plain run's"""
    with _recording(case, "a"):
        full = Run(case, device)
        G = case.grad_like(full.y.detach(), 0)
        gfull = full.backward(G)
        yref, gref = full.reference(G)
        _require_close(case, "a", "y", full.y, yref, "forward, all leaves trainable")
        plain = {}
        for mask in _all_masks(full.leaf):
            label = "{" + ",".join(sorted(mask)) + "}"
            r = Run(case, device, mask=mask)
            _require_bits(case, "a", "y", r.y, full.y, f"forward under mask {label} vs all leaves")
            g = r.backward(G)
            for k in r.leaf:
                if k not in mask:
                    if g[k] is not None:
                        raise ContractError(case.name, "a", k, f"frozen under mask {label} but .grad was written")
                    continue
                _require_close(case, "a", k, g[k], gref[k], f"gradient under mask {label}")
                if k in case.leaves:   # the data gradients do not depend on which parameters train
                    _require_bits(case, "a", k, g[k], gfull[k], f"gradient under mask {label} vs all leaves", gref[k])
            plain[frozenset(mask)] = g
        for mode in modes:   # (label, context manager factory[, used(): a counter that moves when a weight gradient really takes the mode])
            mlabel, ctx, used = mode[0], mode[1], (mode[2] if len(mode) > 2 else None)
            for mask in _all_masks(full.leaf):
                label = "{" + ",".join(sorted(mask)) + "}"
                with ctx():
                    r = Run(case, device, mask=mask)
                    u0 = used() if used else None
                    g = r.backward(G)
                if used and "weight" in mask and not used() > u0:
                    raise ContractError(case.name, "a", "weight", f"control: mask {label} did not take mode {mlabel} (its counter did not move)")
                _require_bits(case, "a", "y", r.y, full.y, f"forward under mask {label}, mode {mlabel}")
                for k in r.leaf:
                    if k not in mask and g[k] is not None:
                        raise ContractError(case.name, "a", k, f"frozen under mask {label}, mode {mlabel}, but .grad was written")
                    if k in mask:
                        _require_bits(case, "a", k, g[k], plain[frozenset(mask)][k], f"gradient under mask {label}: mode {mlabel} vs plain", gref[k])


def grad_forms(G):
    """(label, tensor) hand-overs of G's values in other layouts; all compare equal to G"""
    out = []
    dev, dt = G.device, G.dtype
    if G.dim() == 4:
        n, c, h, w = G.shape
        cl = G.is_contiguous(memory_format=torch.channels_last) and not G.is_contiguous()
        out.append(("other_memory_format", G.contiguous() if cl else G.contiguous(memory_format=torch.channels_last)))
        cw = (c + 7) // 8 * 8 + 16
        for label, off in (("slice_aligned", 8), ("slice_unaligned", 3)):
            wide = torch.zeros((n, cw, h, w), dtype=dt, device=dev).contiguous(memory_format=torch.channels_last)
            wide[:, off:off + c] = G
            out.append((label, wide[:, off:off + c]))
        out.append(("spatial_transposed", G.transpose(2, 3).contiguous().transpose(2, 3)))
    elif G.dim() == 2:
        n, c = G.shape
        wide = torch.zeros((n, c + 24), dtype=dt, device=dev)
        wide[:, 8:8 + c] = G
        out.append(("column_slice", wide[:, 8:8 + c]))
        wide3 = torch.zeros((n, c + 24), dtype=dt, device=dev)
        wide3[:, 3:3 + c] = G
        out.append(("column_slice_unaligned", wide3[:, 3:3 + c]))
        rows = torch.zeros((2 * n, c), dtype=dt, device=dev)
        rows[::2] = G
        out.append(("row_strided", rows[::2]))
        out.append(("transposed_storage", G.t().contiguous().t()))
    else:
        d = G.dim()
        if d == 5:
            cl = G.is_contiguous(memory_format=torch.channels_last_3d) and not G.is_contiguous()
            out.append(("other_memory_format", G.contiguous() if cl else G.contiguous(memory_format=torch.channels_last_3d)))
        if d >= 2:
            out.append(("last_dims_transposed", G.transpose(d - 2, d - 1).contiguous().transpose(d - 2, d - 1)))
            shape = list(G.shape)
            shape[1] += 24
            wide = torch.zeros(shape, dtype=dt, device=dev)
            wide.narrow(1, 8, G.shape[1]).copy_(G)
            out.append(("dim1_slice", wide.narrow(1, 8, G.shape[1])))
    for label, t in out:
        assert t.shape == G.shape and torch.equal(t, G), label
    return out


def contract_grad_forms(case, device):
    """(b)"""
    with _recording(case, "b"):
        base = Run(case, device)
        G = case.grad_like(base.y.detach(), 0)
        g0 = base.backward(G)
        _, gref = base.reference(G)
        for label, form in grad_forms(G):
            r = Run(case, device)
            g = r.backward(form)
            for k in r.leaf:
                _require_bits(case, "b", k, g[k], g0[k], f"upstream gradient as {label} vs dense", gref[k])
        const = torch.full_like(G, 0.5)
        r0 = Run(case, device)
        gc = r0.backward(const)
        _, gcref = r0.reference(const)
        r1 = Run(case, device)
        ge = r1.backward(torch.full((1,) * G.dim(), 0.5, dtype=G.dtype, device=G.device).expand(G.shape))
        for k in r1.leaf:
            _require_bits(case, "b", k, ge[k], gc[k], "upstream gradient as stride-0 expanded constant vs dense constant", gcref[k])


def _state_bits(run):
    st = {f"input:{k}": v for k, v in run.inputs.items() if torch.is_tensor(v)}
    st.update({f"param:{k}": v for k, v in run.module.named_parameters()} if hasattr(run.module, "named_parameters") else {})
    st.update({f"buffer:{k}": v for k, v in run.module.named_buffers()} if hasattr(run.module, "named_buffers") else {})
    return st


def contract_replay(case, device):
    """(c)"""
    with _recording(case, "c"):
        r = Run(case, device)
        G = case.grad_like(r.y.detach(), 0)
        _, gref = r.reference(G)
        live = _state_bits(r)
        before = {k: v.detach().clone() for k, v in live.items()}
        g1 = r.backward(G, retain=True)
        for k, v in live.items():
            _count("bit")
            if not bits_equal(v, before[k]):
                raise ContractError(case.name, "c", k, f"changed by the backward: {_first_diffs(v, before[k])}")
        for t in r.leaf.values():
            t.grad = None
        g2 = r.backward(G, retain=True)
        for k in r.leaf:
            _require_bits(case, "c", k, g2[k], g1[k], "second backward over the retained graph vs the first", gref[k])


def contract_interleave(case, device):
    """(d), first half: fwd A, fwd B, bwd B, bwd A through one module"""
    with _recording(case, "d"):
        iso = {}
        for s in (1, 2):
            r = Run(case, device, seed=s)
            G = case.grad_like(r.y.detach(), s)
            iso[s] = (r.y.detach().clone(), r.backward(G), G, r.reference(G)[1])
        module = case.build(device)
        pnames = list(case.params(module))
        ra = Run(case, device, seed=1, module=module)
        ya = ra.y
        rb = Run(case, device, seed=2, module=module)   # (Run resets the parameters' .grad, nothing else)
        _require_bits(case, "d", "y", ya, iso[1][0], "forward A (before forward B) vs isolated")
        _require_bits(case, "d", "y", rb.y, iso[2][0], "forward B (after forward A) vs isolated")
        gb = rb.backward(iso[2][2])
        for k in rb.leaf:
            _require_bits(case, "d", k, gb[k], iso[2][1][k], "backward B (forward A pending) vs isolated", iso[2][3][k])
        for k in pnames:
            rb.leaf[k].grad = None
        with case.scope():
            ya.backward(iso[1][2])
        case.sync()
        ga = {k: (None if t.grad is None else t.grad.detach().clone()) for k, t in ra.leaf.items()}
        for k in ra.leaf:
            _require_bits(case, "d", k, ga[k], iso[1][1][k], "backward A (after forward B and backward B) vs isolated", iso[1][3][k])


def contract_accumulate(case, device, mode=None, counter=None, used=None):
    """(d), second half: backward A then backward B without zeroing.  mode: context manager factory (side stream on);
    counter(): must move during the second backward when given (the accumulating gradient takes the plain path);
    used(): must move during the FIRST backward when given (control: the mode was really taken, the comparisons are not plain vs plain)"""
    with _recording(case, "d_acc" + ("" if mode is None else "_mode")):
        ctx = mode or contextlib.nullcontext
        with ctx():
            iso = {}
            for s in (1, 2):
                r = Run(case, device, seed=s)
                G = case.grad_like(r.y.detach(), s)
                iso[s] = (r.backward(G), G, r.reference(G)[1])
            module = case.build(device)
            ra = Run(case, device, seed=1, module=module)
            pnames = list(case.params(module))
            if not pnames:   # nothing accumulates in a layer without parameters
                return
            u0 = used() if used else None
            ra.backward(iso[1][1])
            if used and not used() > u0:
                raise ContractError(case.name, "d", pnames[0], "control: the first gradient did not take the mode under test (its counter did not move)")
            with case.scope():
                with case.context():
                    yb = case.call(module, case.inputs(2, device))   # (frozen inputs: only the parameters' gradients accumulate)
                c0 = counter() if counter else None
                yb.backward(iso[2][1])
            case.sync()
            if counter and pnames and not counter() > c0:
                raise ContractError(case.name, "d", pnames[0], "second gradient of a parameter with a pending .grad did not take the plain path")
            for k in pnames:
                want = iso[1][0][k] + iso[2][0][k]
                if k in case.inexact:
                    _require_close(case, "d", k, ra.leaf[k].grad, iso[1][2][k] + iso[2][2][k], "accumulated gradient")
                    continue
                _count("bit")
                if not bits_equal(ra.leaf[k].grad, want):
                    raise ContractError(case.name, "d", k, f"accumulated .grad != gA + gB: {_first_diffs(ra.leaf[k].grad, want)}")


def contract_grad_mode(case, device):
    """(e)"""
    with _recording(case, "e"):
        a = Run(case, device)
        b = Run(case, device, grad_mode=False)
        _require_bits(case, "e", "y", b.y, a.y, "forward under no_grad vs grad mode")
        if b.y.requires_grad:
            raise ContractError(case.name, "e", "y", "output of a no_grad forward requires grad")
        if not case.has_stats and hasattr(a.module, "eval"):
            m = case.build(device).eval()
            c = Run(case, device, module=m)
            _require_bits(case, "e", "y", c.y, a.y, "forward in eval() vs train()")


def contract_param_update(case, device, refresh=None, raw_write=None):
    """(f).  refresh(): the product's hook after a raw-storage write (dense2d.refresh_pack_cache); raw_write(param, values): a write that
    does not bump the version counter"""
    assert case.linear
    with _recording(case, "f"):
        module = case.build(device)
        r1 = Run(case, device, module=module)
        G = case.grad_like(r1.y.detach(), 0)
        g1 = r1.backward(G)
        y1 = r1.y.detach().clone()
        _, gref = r1.reference(G)
        pnames = list(case.params(module))
        with torch.no_grad():
            for p in case.params(module).values():
                p.mul_(2)
        r2 = Run(case, device, module=module)
        g2 = r2.backward(G)
        _require_bits(case, "f", "y", r2.y, (y1.float() * 2).to(y1.dtype), "forward after weight.mul_(2), bias.mul_(2) vs 2 y")
        for k in case.leaves:
            _require_bits(case, "f", k, g2[k], (g1[k].float() * 2).to(g1[k].dtype), "data gradient after the parameters doubled vs 2 dx",
                          None if k not in case.inexact else 2 * gref[k])
        for k in pnames:
            _require_bits(case, "f", k, g2[k], g1[k], "parameter gradient after the parameters doubled vs before", gref[k])
        # new values: the module that ran with the old ones against a freshly built one
        fresh = case.build(device)
        new = {k: (v.detach().clone() * 0.5 if v.dtype.is_floating_point else v.detach().clone()) for k, v in fresh.state_dict().items()}
        fresh.load_state_dict(new)
        rf = Run(case, device, module=fresh)
        gf = rf.backward(G)
        yf = rf.y.detach().clone()
        _, gfref = rf.reference(G)
        writers = [("load_state_dict", lambda m: m.load_state_dict(new))]
        if refresh is not None:
            def raw(m):
                for k, p in list(m.named_parameters()) + list(m.named_buffers()):
                    raw_write(p, new[k])
                refresh()
            writers.append(("raw write + refresh", raw))
        for label, write in writers:
            write(module)
            r3 = Run(case, device, module=module)
            g3 = r3.backward(G)
            _require_bits(case, "f", "y", r3.y, yf, f"forward after {label} vs a fresh module with the same values")
            for k in r3.leaf:
                _require_bits(case, "f", k, g3[k], gf[k], f"gradient after {label} vs a fresh module with the same values", gfref[k])
            with torch.no_grad():   # back to other values, through the ordinary path, so that the next writer has something to change
                for p in module.parameters():
                    p.mul_(2)
            Run(case, device, module=module).backward(G)


def contract_fanout(case, device, label=""):
    """(g): x feeds the layer and an identity skip"""
    with _recording(case, "g" + label):
        alone = Run(case, device)
        G = case.grad_like(alone.y.detach(), 0)
        ga = alone.backward(G)
        _, gref = alone.reference(G)
        r = Run(case, device)
        x = r.leaf["x"]
        gs = torch.Generator().manual_seed(77)
        Gskip = torch.empty_like(x.detach()).copy_(torch.randn(tuple(x.shape), generator=gs).to(x.dtype).to(x.device))
        with case.scope():
            torch.autograd.backward([r.y, x * 1], [G, Gskip])
        case.sync()
        want = ga["x"] + Gskip
        if "x" in case.inexact:
            _require_close(case, "g", "x", x.grad, gref["x"] + Gskip.double().cpu(), "x.grad with an identity skip")
        else:
            _count("bit")
            if not bits_equal(x.grad, want):
                raise ContractError(case.name, "g", "x", f"x.grad != dx_alone + G_skip: {_first_diffs(x.grad, want)}")
        for k in r.leaf:
            if k != "x":
                _require_bits(case, "g", k, r.leaf[k].grad, ga[k], "gradient with an identity skip on x vs alone", gref[k])


class PairCase:
    """producer -> batch norm with the producer's epilogue statistics handed over on the tensor (contract (h)).
    build(device) -> (producer, norm); inputs(seed, device) -> x; produce(producer, x) -> z; norm_call(norm, z) -> y;
    norm_ref(z64, gamma64, beta64) -> y64 (training-mode batch norm [+ activation]); running(norm) -> dict of running statistics;
    running_ref(z64, norm_before) -> dict; counter() -> forwards that consumed a tag; tol: "y", "z", "gamma", "beta", "running"."""

    def __init__(self, name, build, inputs, produce, norm_call, norm_params, norm_ref, running, running_ref, counter, tol,
                 context=contextlib.nullcontext, sync=None):
        self.name, self.build, self.inputs, self.produce, self.norm_call, self.norm_params = name, build, inputs, produce, norm_call, norm_params
        self.norm_ref, self.running, self.running_ref, self.counter, self.tol, self.context = norm_ref, running, running_ref, counter, tol, context
        self.sync = sync or (lambda: None)
        self.inexact = frozenset()


INPLACE_OPS = {"none": None, "add_": lambda z: z.add_(0.75), "mul_": lambda z: z.mul_(-1.5), "relu_": lambda z: z.relu_()}


def contract_stale_tags(case, device, op):
    """(h).  op = "none" is the control: the tag must be consumed (the counter moves); after an in-place op it must not be"""
    with _recording(case, "h:" + op):
        producer, norm = case.build(device)
        x = case.inputs(0, device).requires_grad_(True)
        run0 = {k: v.detach().double().cpu().clone() for k, v in case.running(norm).items()}
        c0 = case.counter()
        with case.context():
            z = case.produce(producer, x)
            if INPLACE_OPS[op] is not None:
                z = INPLACE_OPS[op](z)
            z.retain_grad()
            y = case.norm_call(norm, z)
        moved = case.counter() - c0
        if op == "none" and moved != 1:
            raise ContractError(case.name, "h", "y", f"control: the producer's epilogue statistics were not consumed (counter moved by {moved})")
        if op != "none" and moved != 0:
            raise ContractError(case.name, "h", "y", f"statistics of the tensor before {op} were consumed (counter moved by {moved})")
        G = default_grad(y.detach(), 0)
        y.backward(G)
        case.sync()
        z64 = z.detach().double().cpu().requires_grad_(True)
        p64 = {k: p.detach().double().cpu().requires_grad_(True) for k, p in case.norm_params(norm).items()}
        yr = case.norm_ref(z64, p64["gamma"], p64["beta"])
        gz, gg, gb = torch.autograd.grad(yr, [z64, p64["gamma"], p64["beta"]], G.double().cpu())
        _require_close(case, "h", "y", y, yr.detach(), f"norm output after {op} vs float64 on the modified tensor")
        _require_close(case, "h", "z", z.grad, gz, f"norm input gradient after {op}")
        params = case.norm_params(norm)
        _require_close(case, "h", "gamma", params["gamma"].grad, gg, f"gamma gradient after {op}")
        _require_close(case, "h", "beta", params["beta"].grad, gb, f"beta gradient after {op}")
        want = case.running_ref(z64.detach(), run0)
        for k, v in case.running(norm).items():
            a, r = v.detach().double().cpu(), want[k]
            # running statistics are held RELATIVE TO THE MOVE this forward made (momentum * batch statistic), not to the large resting value
            move = (r - run0[k]).abs().max()
            err = float((a - r).abs().max())
            bound = case.tol["running"] * float(move)
            _count("tol", err / bound if bound > 0 else 0.0)
            if not err <= bound:
                raise ContractError(case.name, "h", k, f"after {op}: |err| {err:.4g} > {case.tol['running']:g} * |update| = {bound:.4g}")
