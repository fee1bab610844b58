"""The shape-static dense segment replayed as HIP graphs (sparse2dense_amd/graphed.py, `detector.use_hip_graphs()`): the same kernels on the
same operands in the same order as the kernel-by-kernel run, so a training run must not depend on the mode - bit-identical losses,
parameters and gradients - whether the segment is the S2D student's (S2D module + PCR head with padded recon-voxel lists + RPN trunk +
CenterHead + losses), plain CenterPoint's, or the frozen distillation teacher's forward-only graph.
Reference loop: /root/reference/det3d/torchie/trainer/trainer.py:775-811, hooks/optimizer.py:15-21."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(kind, dev):
    from sparse2dense_amd import waymo_configs
    from sparse2dense_amd.registry import build_detector
    m = build_detector(getattr(waymo_configs, kind)())
    m.dense_dtype = torch.bfloat16
    m.use_channels_last()
    return m.to(dev)


def _run(graph, steps=6, n_points=12000, batch=2, kind="s2d_student", vary=False, fork="", defer="dense,aux,pcr", split="0"):
    from sparse2dense_amd import dense2d, graphed, hip_ops, side
    from sparse2dense_amd.data import SyntheticFrames
    from sparse2dense_amd.solver import build_one_cycle_optimizer, build_one_cycle_scheduler
    from sparse2dense_amd.train_step import backward_and_step
    import os
    os.environ["S2D_GRAPH_SPLIT"] = split   # "1": the S2D student's dense part as two graphed segments in sequence (detectors.KD_VoxelNet._dense_call)
    side.enable(False)
    side.graph_fork(fork if fork else False)
    side.graph_defer(defer if defer else False)
    side.stats["deferred"] = 0
    dense2d.clear_pack_cache()
    hip_ops.set_sparse_compute_dtype("s16")
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    model = _model(kind, dev).train()
    if graph:
        model.use_hip_graphs()
    distill = kind == "s2d_student"
    sets = [SyntheticFrames(batch, n_points=n_points + 1500 * k, seed=5 + 10 * k, distill=distill, device=dev) for k in range(3 if vary else 1)]
    params = [p for p in model.parameters() if p.requires_grad]
    opt = build_one_cycle_optimizer(model, dict(wd=0.01))
    sch = build_one_cycle_scheduler(opt, dict(type="one_cycle", lr_max=0.003, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), total_steps=100)
    for k in graphed.stats:
        graphed.stats[k] = 0
    losses = []
    try:
        for it in range(steps):
            ex = sets[it % len(sets)].example()
            if distill:
                out = model(ex, return_loss=True, return_feature=True)
                loss = sum(out[0]["loss"]) + out[4] + out[5]
            else:
                loss = sum(model(ex, return_loss=True)["loss"])
            if it == steps - 1:   # last step by hand: the gradients themselves are compared
                for p in params:
                    p.grad = None
                loss.backward()
                torch.cuda.synchronize()
                grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
            else:
                backward_and_step(loss, params, opt, sch, it, 35.0)
            losses.append(float(loss))
        final = torch.cat([p.detach().flatten()[:64].double().cpu() for p in params])
        bn = torch.cat([b.detach().flatten()[:16].double().cpu() for b in model.buffers()])
        st = dict(graphed.stats)
    finally:
        os.environ.pop("S2D_GRAPH_SPLIT", None)
        side.graph_fork(False)
        side.graph_defer("dense,aux,pcr")
        hip_ops.set_sparse_compute_dtype("f32")
        dense2d.clear_pack_cache()
    return losses, final, grads, bn, st


_REF_RUNS = {}


def _eager_ref(kind="s2d_student"):
    """the kernel-by-kernel run of the default settings, computed once per detector kind (every parametrisation compares against the same run)"""
    if kind not in _REF_RUNS:
        _REF_RUNS[kind] = _run(False, kind=kind)
        assert _REF_RUNS[kind][4]["replay"] == 0
    return _REF_RUNS[kind]


def _same(a, b, what):
    la, fa, ga, ba, _ = a
    lb, fb, gb, bb, _ = b
    assert la == lb, (what, la, lb)
    assert torch.equal(fa, fb), what
    assert torch.equal(ba, bb), what + ": batch-norm running statistics"
    for g, r in zip(ga, gb):
        assert (g is None) == (r is None), what
        if g is not None:
            assert torch.equal(g, r), what


@pytest.mark.parametrize("kind,split", [("s2d_student", "1"), ("s2d_student", "0"), ("centerpoint_voxelnet", "1")])
@pytest.mark.parametrize("defer", ["dense,aux,pcr", "dense,aux", ""])
def test_training_run_is_independent_of_the_graph_replay(kind, split, defer):
    """defer = the layer kinds whose weight gradients are captured into a second graph that is replayed on the side stream beside the eager
    sparse backward (side.GRAPH_DEFER, the default); "" = everything in the chain's graph"""
    from sparse2dense_amd import side
    ref = _eager_ref(kind)
    got = _run(True, kind=kind, defer=defer, split=split)
    segs = 2 if (kind == "s2d_student" and split == "1") else 1
    assert got[4]["capture"] == segs and got[4]["replay"] == 4 * segs, got[4]    # 2 eager warm-up calls, then capture + replays
    assert (side.stats["deferred"] > 20) == bool(defer), side.stats
    _same(got, ref, kind)
    assert ref[0][-1] != ref[0][0]


def test_training_step_declares_its_gradients_consumed_and_nothing_is_parked():
    """r06: `train_step.backward_and_step` calls `graphed.grads_consumed()` after the optimizer has read the gradients, so the next forward replay
    does not move the 164 static gradient buffers that are still bound as `.grad` to private copies (0.64 ms of copy kernels + ~1.6 ms of launch-
    thread time per step in the graphed mode before) - and the run stays bit-equal to the kernel-by-kernel one.  Without the declaration (the
    accumulation test below) they are parked."""
    got = _run(True)
    _same(got, _eager_ref(), "graphed training steps with consumed gradients")
    assert got[4]["replay"] > 0 and got[4]["parked"] == 0, got[4]


def test_weight_gradients_as_branches_of_the_backward_graph():
    """side.graph_fork("dense,aux"): inside the capture the weight-gradient launch groups fork onto a second capturing stream and rejoin
    at the end - parallel branches of the replayed backward graph; same kernels, same operands: bit-equal to the kernel-by-kernel run"""
    from sparse2dense_amd import side
    ref = _eager_ref()
    side.stats["forked"] = 0
    got = _run(True, fork="dense,aux", defer="", split="0")
    assert side.stats["forked"] > 20, side.stats
    assert got[4]["capture"] == 1 and got[4]["replay"] == 4, got[4]
    _same(got, ref, "forked weight gradients")


def test_graph_replay_with_recon_lists_of_changing_length():
    """three point clouds of different sizes in rotation: the sparse stack is eager and re-planned per cloud, the PCR head's recon-voxel lists
    shrink and grow inside their padded buffers, the dense graphs are captured once"""
    ref = _run(False, steps=8, vary=True)
    got = _run(True, steps=8, vary=True)
    assert got[4]["capture"] == 1 and got[4]["replay"] == 6, got[4]
    _same(got, ref, "varying clouds")


def test_parameter_surgery_drops_the_capture():
    """load_state_dict (version counters move) behind a captured segment: the next call must not replay a graph that reads stale packed
    weight images - it re-runs eagerly and captures again"""
    from sparse2dense_amd import dense2d, graphed, hip_ops
    from sparse2dense_amd.data import SyntheticFrames
    hip_ops.set_sparse_compute_dtype("s16")
    dense2d.clear_pack_cache()
    dev = torch.device("cuda:0")
    try:
        torch.manual_seed(3)
        model = _model("centerpoint_voxelnet", dev).train().use_hip_graphs()
        twin = _model("centerpoint_voxelnet", dev).train()
        frames = SyntheticFrames(1, n_points=9000, seed=2, device=dev)
        for k in graphed.stats:
            graphed.stats[k] = 0

        def loss_of(m):
            return float(sum(m(frames.example(), return_loss=True)["loss"]))
        for _ in range(4):
            loss_of(model)
        assert graphed.stats["capture"] == 1 and graphed.stats["replay"] == 2
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        torch.manual_seed(99)
        for p in model.parameters():
            sd_key = [k for k, v in model.named_parameters() if v is p][0]
            sd[sd_key] = sd[sd_key] + 0.01 * torch.randn_like(p)
        model.load_state_dict(sd)
        twin.load_state_dict(sd)
        a = loss_of(model)
        assert graphed.stats["dropped"] == 1
        twin.load_state_dict(model.state_dict())   # (running statistics moved by the calls above)
        b = loss_of(twin)
        assert a == b, (a, b)
    finally:
        hip_ops.set_sparse_compute_dtype("f32")
        dense2d.clear_pack_cache()


def _run_distill(graph, steps=6, n_points=12000, batch=2):
    """the full distillation step (trainer.py:775-811): frozen teacher forward (a forward-only graph under no_grad) + student step whose
    feature maps and predictions ALSO receive gradients (sparse2dense_loss, kd_hm, kd_reg on top of the detection and PCR losses)"""
    from sparse2dense_amd import dense2d, graphed, hip_ops, side
    from sparse2dense_amd.data import SyntheticFrames
    from sparse2dense_amd.solver import build_one_cycle_optimizer, build_one_cycle_scheduler
    from sparse2dense_amd.train_step import backward_and_step, distill_loss
    side.enable(False)
    side.graph_defer("dense,aux,pcr")
    dense2d.clear_pack_cache()
    hip_ops.set_sparse_compute_dtype("s16")
    dev = torch.device("cuda:0")
    torch.manual_seed(21)
    student = _model("s2d_student", dev).train()
    teacher = _model("centerpoint_voxelnet", dev).eval()
    for p in teacher.parameters():
        p.requires_grad = False
    if graph:
        student.use_hip_graphs()
        teacher.use_hip_graphs()
    frames = SyntheticFrames(batch, n_points=n_points, seed=8, distill=True, device=dev)
    params = [p for p in student.parameters() if p.requires_grad]
    opt = build_one_cycle_optimizer(student, dict(wd=0.01))
    sch = build_one_cycle_scheduler(opt, dict(type="one_cycle", lr_max=0.003, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), total_steps=100)
    for k in graphed.stats:
        graphed.stats[k] = 0
    out = []
    try:
        for it in range(steps):
            loss, terms = distill_loss(teacher, student, frames.example())
            out.append((float(loss.detach()), float(terms["sparse2dense_loss"][0]), float(terms["kd_hm_loss"][0]), float(terms["kd_reg_loss"][0])))
            if it == steps - 1:
                for p in params:
                    p.grad = None
                loss.backward()
                torch.cuda.synchronize()
                grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
            else:
                backward_and_step(loss, params, opt, sch, it, 35.0)
        final = torch.cat([p.detach().flatten()[:64].double().cpu() for p in params])
        st = dict(graphed.stats)
    finally:
        hip_ops.set_sparse_compute_dtype("f32")
        dense2d.clear_pack_cache()
    return out, final, grads, st


def test_distillation_step_is_independent_of_the_graph_replay():
    ref_out, ref_final, ref_grads, st0 = _run_distill(False)
    got_out, got_final, got_grads, st = _run_distill(True)
    assert st0["replay"] == 0 and st["capture"] == 2 and st["replay"] == 8, st   # teacher (forward only) + student segments, 4 replays each
    assert got_out == ref_out, (got_out, ref_out)
    assert torch.equal(got_final, ref_final)
    for g, r in zip(got_grads, ref_grads):
        assert (g is None) == (r is None)
        if g is not None:
            assert torch.equal(g, r)
    assert ref_out[-1][0] != ref_out[0][0] and ref_out[0][1] > 0 and ref_out[0][2] > 0


def test_graph_replay_with_the_batch_norm_collectives_captured_inside_on_one_rank(monkeypatch):
    """the N>1 route at world_size 1 over RCCL (dp.wrap_ddp -> gradient buckets, self-synchronising batch norms on the library's own RCCL
    communicator, collective.init_direct) with S2D_DENSE_GRAPH_SYNCBN=1: every batch-norm all-reduce of the dense segment is a node of the
    forward / backward HIP graph (capture mode thread_local: c10d's watchdog thread polls its events while the capture runs), the gradient
    buckets fire from the hooks `_Replay.backward` runs - and the run equals the kernel-by-kernel one bit for bit.
    Reference: /root/reference/det3d/torchie/apis/train.py:360-391 (SyncBN + DistributedDataParallel)."""
    import torch.distributed as dist
    from sparse2dense_amd import _lib, collective, dense2d, dp, graphed, hip_ops, side, waymo_configs
    from sparse2dense_amd.data import SyntheticFrames
    from sparse2dense_amd.registry import build_detector
    from sparse2dense_amd.solver import build_one_cycle_optimizer, build_one_cycle_scheduler
    from sparse2dense_amd.train_step import backward_and_step
    if dist.is_initialized():
        pytest.skip("a process group is already up")
    monkeypatch.setenv("S2D_FORCE_DDP", "1")
    monkeypatch.setenv("S2D_BUCKET_MB", "4")
    monkeypatch.setenv("S2D_DENSE_GRAPH_SYNCBN", "1")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29593", rank=0, world_size=1)
    dev = torch.device("cuda:0")

    def run(graph, steps=6):
        side.enable(False)
        side.graph_defer("dense,aux,pcr")
        dense2d.clear_pack_cache()
        hip_ops.set_sparse_compute_dtype("s16")
        torch.manual_seed(11)
        model = build_detector(waymo_configs.s2d_student())
        model.dense_dtype = torch.bfloat16
        model.use_channels_last()
        model = dp.wrap_ddp(model.to(dev).train(), 0)
        assert collective.sync_on() and collective.direct_enabled()
        if graph:
            getattr(model, "module", model).use_hip_graphs()
        frames = SyntheticFrames(2, n_points=12000, seed=5, distill=True, device=dev)
        params = [p for p in model.parameters() if p.requires_grad]
        opt = build_one_cycle_optimizer(model, dict(wd=0.01))
        sch = build_one_cycle_scheduler(opt, dict(type="one_cycle", lr_max=0.003, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), total_steps=100)
        for k in graphed.stats:
            graphed.stats[k] = 0
        losses = []
        for it in range(steps):
            out = model(frames.example(), return_loss=True, return_feature=True)
            loss = sum(out[0]["loss"]) + out[4] + out[5]
            backward_and_step(loss, params, opt, sch, it, 35.0)
            losses.append(float(loss.detach()))
        final = torch.cat([p.detach().flatten()[:64].double().cpu() for p in params])
        model._s2d_grad_buckets.remove()
        return losses, final, dict(graphed.stats)
    try:
        ref = run(False)
        got = run(True)
        assert ref[2]["replay"] == 0 and got[2]["capture"] == 1 and got[2]["replay"] == 4, (ref[2], got[2])
        assert got[0] == ref[0], (got[0], ref[0])
        assert torch.equal(got[1], ref[1])
        assert ref[0][-1] != ref[0][0]
    finally:
        hip_ops.set_sparse_compute_dtype("f32")
        dense2d.clear_pack_cache()
        collective._DIRECT = False
        _lib.load().s2d_comm_shutdown()
        dist.destroy_process_group()


def _eval_between_training_steps(graph):
    """train 2 steps -> eval x 4 (graph: 2 eager warm-up calls, capture, replay) -> train 1 step -> eval x 2 (replays): the evaluation outputs"""
    from sparse2dense_amd import dense2d, graphed, hip_ops, side
    from sparse2dense_amd.data import SyntheticFrames
    from sparse2dense_amd.solver import build_one_cycle_optimizer, build_one_cycle_scheduler
    from sparse2dense_amd.train_step import backward_and_step
    side.enable(False)
    dense2d.clear_pack_cache()
    hip_ops.set_sparse_compute_dtype("s16")
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    model = _model("s2d_student", dev).train()
    if graph:
        model.use_hip_graphs()
    frames = SyntheticFrames(2, n_points=12000, seed=5, distill=True, device=dev)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = build_one_cycle_optimizer(model, dict(wd=0.01))
    sch = build_one_cycle_scheduler(opt, dict(type="one_cycle", lr_max=0.003, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), total_steps=100)
    for k in graphed.stats:
        graphed.stats[k] = 0
    outs, it = [], 0

    def train(n):
        nonlocal it
        model.train()
        for _ in range(n):
            out = model(frames.example(), return_loss=True, return_feature=True)
            backward_and_step(sum(out[0]["loss"]) + out[4] + out[5], params, opt, sch, it, 35.0)
            it += 1

    def evaluate(n):
        model.eval()
        with torch.no_grad():
            for _ in range(n):
                out = model(frames.example(), return_loss=True, return_feature=True)   # eval mode: no PCR branch, forward-only segment
                outs.append((out[1].float().clone(), out[2].float().clone()))
    try:
        train(2)
        evaluate(4)
        train(1)
        evaluate(2)
        torch.cuda.synchronize()
        st = dict(graphed.stats)
    finally:
        hip_ops.set_sparse_compute_dtype("f32")
        dense2d.clear_pack_cache()
    return outs, st


def test_forward_only_capture_with_a_warm_pack_cache_survives_optimizer_steps():
    """an evaluation capture taken with a WARM packed-weight cache baked in the addresses of images that have no in-place refresh
    (layer-norm / 1x1 matrices); the next optimizer step freed them (the fused Adam writes through raw pointers: the capture's staleness check
    sees nothing) and the replay read freed memory.  The capture now builds such images inside itself (dense2d.CAPTURE_PACKS)."""
    ref, st0 = _eval_between_training_steps(False)
    got, st = _eval_between_training_steps(True)
    assert st0["replay"] == 0 and st["replay"] >= 4 and st["capture"] >= 2, st
    for k, ((a1, b1), (a0, b0)) in enumerate(zip(got, ref)):
        assert torch.equal(a1, a0) and torch.equal(b1, b0), f"evaluation call {k} differs from the kernel-by-kernel run"
    assert not torch.equal(ref[3][0], ref[5][0])   # the training step in between did move the weights


def _two_backwards(graph):
    from sparse2dense_amd import dense2d, graphed, hip_ops, side
    from sparse2dense_amd.data import SyntheticFrames
    side.enable(False)
    dense2d.clear_pack_cache()
    hip_ops.set_sparse_compute_dtype("s16")
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    model = _model("s2d_student", dev).train()
    if graph:
        model.use_hip_graphs()
    sets = [SyntheticFrames(2, n_points=12000, seed=5 + 10 * k, distill=True, device=dev) for k in range(2)]
    params = [p for p in model.parameters() if p.requires_grad]

    def loss_of(k):
        out = model(sets[k].example(), return_loss=True, return_feature=True)
        return sum(out[0]["loss"]) + out[4] + out[5]
    singles = []
    try:
        for _ in range(3):   # warm-up calls + capture, one backward each
            for p in params:
                p.grad = None
            loss_of(0).backward()
        for k in (0, 1):     # each micro-batch on its own (diagnostics: which sum did a wrong accumulation produce?)
            for p in params:
                p.grad = None
            loss_of(k).backward()
            side.join()
            torch.cuda.synchronize()
            singles.append([None if p.grad is None else p.grad.detach().clone() for p in params])
        for p in params:
            p.grad = None
        loss_of(0).backward()
        loss_of(1).backward()          # second micro-batch: accumulates onto the first
        side.join()
        torch.cuda.synchronize()
        grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
        for p in params:               # ... and the zero_grad(set_to_none=False) pattern: .grad stays bound and is zeroed in place
            if p.grad is not None:
                p.grad.zero_()
        loss_of(1).backward()
        side.join()
        torch.cuda.synchronize()
        grads2 = [None if p.grad is None else p.grad.detach().clone() for p in params]
    finally:
        hip_ops.set_sparse_compute_dtype("f32")
        dense2d.clear_pack_cache()
    return grads, grads2, singles, [n for n, p in model.named_parameters() if p.requires_grad]


def test_gradient_accumulation_over_two_backward_passes_matches_the_eager_run():
    """the first backward binds p.grad to the capture's static buffer; a second backward replayed into that very buffer and then
    added it to itself (2 x the second gradient, the first lost).  Now: the bound values are copied out before the replay."""
    ref, ref2, ref_single, names = _two_backwards(False)
    got, got2, got_single, _ = _two_backwards(True)
    for k in (0, 1):   # the single passes agree (what the other graph tests hold) ...
        for n, g, r in zip(names, got_single[k], ref_single[k]):
            assert (g is None) == (r is None) and (g is None or torch.equal(g, r)), ("single backward", k, n)
    for what, pair in (("two backwards", (got, ref)), ("zeroed in place + one backward", (got2, ref2))):
        for i, (n, g, r) in enumerate(zip(names, *pair)):
            assert (g is None) == (r is None), n
            if g is not None and not torch.equal(g, r):   # eager accumulates in place (a += b), the graph path out of place (a + b): the same fp32 sum
                rel = lambda a, b: float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
                s0, s1 = ref_single[0][i], ref_single[1][i]
                raise AssertionError((what, n, "vs eager sum", rel(g, r), "vs 2 x second", rel(g, 2 * s1), "vs second", rel(g, s1), "vs first", rel(g, s0)))


# ---- gradient accumulation patterns: graph replay against the kernel-by-kernel run and against a float64 sum of single passes ----------
# Every capture of a segment records into ONE memory pool: a block that holds a static gradient buffer (bound as `.grad`) or a saved
# activation of one capture can be a temporary of another capture's graphs.  Each pattern below runs twice - graphed and with graphs off -
# and must be (a) bit-equal between the two (gradients, losses, outputs, input gradients) and (b) within rel 1e-6 of the float64 sum of the
# micro-batches' gradients taken one by one on fresh `.grad` tensors.  The graphed run must also replay exactly as the protocol says
# (graphed.stats against `_protocol`), so that a segment which silently went eager cannot pass.

def _protocol(calls, max_caps=None, warmup=None):
    """the graphed.stats a GraphedSegment should produce for a sequence of (signature key, runs eagerly because a backward is pending)"""
    from sparse2dense_amd import graphed
    max_caps = graphed.MAX_CAPTURES if max_caps is None else max_caps
    warmup = graphed.WARMUP if warmup is None else warmup
    caps, seen, st = [], {}, dict(eager=0, capture=0, replay=0, dropped=0)
    for key, conflict in calls:
        if key in caps:
            caps.remove(key)
            caps.append(key)
        elif seen.get(key, 0) < warmup:
            seen[key] = seen.get(key, 0) + 1
            st["eager"] += 1
            continue
        if conflict:
            st["eager"] += 1
            continue
        if key not in caps:
            caps.append(key)
            while len(caps) > max_caps:
                seen.pop(caps.pop(0), None)
                st["dropped"] += 1
            st["capture"] += 1
        st["replay"] += 1
    return st


def _grads(params):
    from sparse2dense_amd import side
    side.join()
    torch.cuda.synchronize()
    return [None if p.grad is None else p.grad.detach().clone() for p in params]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _check_sums(what, got, ref, terms, names):
    """got / ref: the graphed / kernel-by-kernel accumulated gradients; terms: the single micro-batch gradients of the graphed run (bit-equal to
    the kernel-by-kernel ones: asserted where they are taken) whose float64 sum both must match"""
    for i, n in enumerate(names):
        g, r = got[i], ref[i]
        assert (g is None) == (r is None), (what, n)
        if g is None:
            continue
        parts = [t[i] for t in terms if t[i] is not None]
        want = sum(t.double() for t in parts)
        if not torch.equal(g, r):   # eager accumulates in place (a += b), the graph path out of place (a + b): the same fp32 sum
            raise AssertionError((what, n, "vs eager", _rel(g, r), "vs float64 sum", _rel(g, want), "vs 2 x last", _rel(g, 2 * parts[-1]),
                                  "vs last", _rel(g, parts[-1]), "vs first", _rel(g, parts[0])))
        err = _rel(g, want)
        assert err <= 1e-6 and (want.norm() > 0 or not g.any()), (what, n, "vs float64 sum of the single passes", err)


class _Toy:
    """a small GraphedSegment of the library's 2-D layers (bf16 channels-last conv 3x3 / 1x1 + batch norm + ReLU) with a scalar loss.  Every
    activation and every parameter gradient is below 1 MB: all come from the allocator's small-block pool, where one capture's gradient
    buffers land on the blocks another capture's temporaries were freed to."""

    SIGS = {"A": (2, 40, 48), "B": (1, 56, 40), "C": (3, 24, 32)}

    def __init__(self, seed=7):
        from sparse2dense_amd import dense2d as D, graphed
        dev = torch.device("cuda:0")
        torch.manual_seed(seed)
        bn = lambda c: D.FastBatchNorm2d(c, eps=1e-3, momentum=0.01)
        self.net = torch.nn.Sequential(*D.fuse_bn_relu([
            D.Conv3x3(64, 64, 3, padding=1, bias=False), bn(64), torch.nn.ReLU(),
            D.Conv1x1(64, 128, 1, bias=False), bn(128), torch.nn.ReLU(),
            D.Conv3x3(128, 128, 3, padding=1, bias=False), bn(128), torch.nn.ReLU(),
            D.Conv1x1(128, 64, 1, bias=True), bn(64), torch.nn.ReLU()])).to(dev).train()
        with torch.no_grad():
            for m in self.net:
                if isinstance(m, D.FastBatchNorm2d):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.5, 0.5)
        self.params = [p for p in self.net.parameters() if p.requires_grad]
        self.names = [n for n, p in self.net.named_parameters() if p.requires_grad]
        self.seg = graphed.GraphedSegment(self._fn, [self.net], name=f"toy{seed}")
        self.data = {}
        for k, (sig, (n, h, w)) in enumerate((f"{s}{j}", self.SIGS[s]) for s in "ABC" for j in (0, 1)):
            g = torch.Generator().manual_seed(100 * seed + k)
            x = torch.randn(n, 64, h, w, generator=g).to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)
            t = torch.randn(n, 64, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
            self.data[sig] = (x, t)
        self.calls, self.outs, self.xgrads = [], [], []

    def _fn(self, x, t):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = self.net(x)
        return ((y.float() - t).square().mean()), y

    def loss(self, mb, conflict=False):
        """one segment call on micro-batch `mb` ("A0", "B1", ...); conflict: a backward of this segment is pending - the call runs eagerly"""
        x, t = self.data[mb]
        x = x.clone().requires_grad_(torch.is_grad_enabled())
        self.calls.append(((mb[0], torch.is_grad_enabled()), conflict))
        loss, y = self.seg(x, t)
        self.outs.append((loss.detach().clone(), y.detach().clone()))   # (outputs are static buffers: valid until the segment's next call)
        if x.requires_grad:
            self.xgrads.append(x)
        return loss

    def single(self, mb):
        for p in self.params:
            p.grad = None
        self.loss(mb).backward()
        return _grads(self.params)

    def capture(self, mb):
        """warm-up calls + capture of mb's signature, one backward each: every pass must give the same gradient; returns it"""
        runs = [self.single(mb) for _ in range(3)]
        for r in runs[1:]:
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(r, runs[0])), ("eager warm-up vs replay", mb)
        return runs[-1]

    def record(self):
        return dict(outs=[(a.cpu(), b.float().cpu()) for a, b in self.outs],
                    xgrads=[None if x.grad is None else x.grad.float().cpu() for x in self.xgrads])


def _toy_run(graph, body, monkeypatch, n_models=1):
    """body(toys) -> {name: (accumulated gradients, [single-pass gradients they must sum])}"""
    from sparse2dense_amd import dense2d, graphed, side
    monkeypatch.setenv("S2D_DENSE_GRAPH", "1" if graph else "0")
    side.enable(False)
    side.graph_defer("dense,aux,pcr")   # (the default: the conv weight gradients come out of the side-stream graph)
    dense2d.clear_pack_cache()
    for k in graphed.stats:
        graphed.stats[k] = 0
    try:
        toys = [_Toy(seed=7 + 6 * i) for i in range(n_models)]
        res = body(toys)
        torch.cuda.synchronize()
        st = dict(graphed.stats)
    finally:
        dense2d.clear_pack_cache()
    return res, [t.record() for t in toys], [t.calls for t in toys], st, toys[0].names


def _toy_compare(body, monkeypatch, n_models=1, conflicts=0, max_caps=None):
    got, got_rec, calls, st, names = _toy_run(True, body, monkeypatch, n_models)
    ref, ref_rec, _, st0, _ = _toy_run(False, body, monkeypatch, n_models)
    assert st0["replay"] == 0 and st0["capture"] == 0, st0
    for what in got:
        for gs, rs in zip(got[what][1], ref[what][1]):   # the single passes themselves
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(gs, rs)), (what, "single pass")
        _check_sums(what, got[what][0], ref[what][0], got[what][1], names)
    for k, (a, b) in enumerate(zip(got_rec, ref_rec)):
        assert len(a["outs"]) == len(b["outs"])
        for i, ((la, ya), (lb, yb)) in enumerate(zip(a["outs"], b["outs"])):
            assert torch.equal(la, lb) and torch.equal(ya, yb), ("outputs of call", k, i)
        for i, (ga, gb) in enumerate(zip(a["xgrads"], b["xgrads"])):
            assert (ga is None) == (gb is None) and (ga is None or torch.equal(ga, gb)), ("input gradient of call", k, i)
    want = dict(eager=0, capture=0, replay=0, dropped=0)
    for c in calls:
        for k, v in _protocol(c, max_caps).items():
            want[k] += v
    assert {k: st[k] for k in want} == want, (st, want)
    assert sum(c for cs in calls for _, c in cs) == conflicts
    assert st["replay"] > 0
    return st


def _accumulate(toy, *mbs, zero_in_place=False):
    for p in toy.params:
        if zero_in_place and p.grad is not None:
            p.grad.zero_()
        else:
            p.grad = None
    for mb in mbs:
        toy.loss(mb).backward()
    return _grads(toy.params)


def test_accumulation_over_two_captured_signatures(monkeypatch):
    """two signatures (a last micro-batch with fewer frames): A and B captured in that order, then B's backward binds B's static gradient
    buffers as .grad and A's replays run over them - in both orders, and with zero_grad(set_to_none=False) in between"""
    def body(toys):
        toy = toys[0]
        sa, sb = toy.capture("A0"), toy.capture("B0")
        out = {"B then A": (_accumulate(toy, "B0", "A0"), [sb, sa]),
               "A then B": (_accumulate(toy, "A0", "B0"), [sa, sb])}
        out["zeroed in place, B then A"] = (_accumulate(toy, "B0", "A0", zero_in_place=True), [sb, sa])
        out["zeroed in place, A then B"] = (_accumulate(toy, "A0", "B0", zero_in_place=True), [sa, sb])
        return out
    st = _toy_compare(body, monkeypatch)
    assert st["capture"] == 2 and st["replay"] == 10, st


def test_accumulation_while_captures_are_evicted(monkeypatch):
    """MAX_CAPTURES = 2 and three signatures in rotation while the gradients accumulate: captures are dropped and taken again while their
    static gradient buffers are still somebody's .grad"""
    from sparse2dense_amd import graphed
    monkeypatch.setattr(graphed, "MAX_CAPTURES", 2)

    def body(toys):
        toy = toys[0]
        s = {mb: toy.capture(mb) for mb in ("A0", "B0", "C0")}   # C's capture drops A's
        seq = ["B0", "C0", "A0", "A0", "A0", "B0", "B0", "B0", "C0", "A0"]   # A comes back (drops B), B comes back (drops C), ...
        return {"rotation": (_accumulate(toy, *seq), [s[mb] for mb in seq])}
    st = _toy_compare(body, monkeypatch, max_caps=2)
    assert st["dropped"] >= 3, st


@pytest.mark.parametrize("pair", ["A0+A1", "A0+B0", "B0+A0"])
def test_two_forwards_then_one_backward_of_the_summed_loss(pair, monkeypatch):
    """loss = f(x1) + f(x2); loss.backward(): the second forward must not replay over the activations the first call's backward reads (same
    signature: the same static buffers; another signature: the same pool) - it runs eagerly, and only it"""
    first, second = pair.split("+")

    def body(toys):
        toy = toys[0]
        s = {mb: toy.capture(mb) for mb in ("A0", "B0")}
        s["A1"] = toy.single("A1")
        out = {}
        for rnd in range(2):
            for p in toy.params:
                p.grad = None
            (toy.loss(first) + toy.loss(second, conflict=True)).backward()
            out[f"{pair} #{rnd}"] = (_grads(toy.params), [s[first], s[second]])
        out["one more call after it"] = (toy.single(second), [s[second]])   # (replays again)
        return out
    st = _toy_compare(body, monkeypatch, conflicts=2)
    assert st["replay"] == 6, st


def test_forward_only_calls_between_backwards_and_before_the_optimizer_read(monkeypatch):
    """an evaluation call (no_grad, eval) of the same segment, captured BEFORE the training capture, replayed between a backward and the read
    of its gradients, and between two accumulated backwards"""
    def evaluate(toy, mb):
        toy.net.eval()
        with torch.no_grad():
            toy.loss(mb)
        toy.net.train()

    def body(toys):
        toy = toys[0]
        for _ in range(3):
            evaluate(toy, "A1")
        s = {"A0": toy.capture("A0"), "B0": toy.capture("B0")}
        out = {}
        for p in toy.params:
            p.grad = None
        toy.loss("A0").backward()
        evaluate(toy, "B1")
        evaluate(toy, "A1")
        out["backward, evaluation, read"] = (_grads(toy.params), [s["A0"]])
        for p in toy.params:
            p.grad = None
        toy.loss("B0").backward()
        evaluate(toy, "A1")
        toy.loss("A0").backward()
        out["backward, evaluation, backward"] = (_grads(toy.params), [s["B0"], s["A0"]])
        return out
    _toy_compare(body, monkeypatch)


_STALE_MEAN = ("model 2's segment replayed twice before model 1's segment was captured: model 1's `.mean()` loss output (a full reduction of "
               "a channels-last fp32 tensor) keeps the value of its first replay on every later replay, while y, the input gradient and the "
               "weight gradients of the same replays are right and `.sum() / numel()` in its place is right too; not reproduced with a bare "
               "torch graph of the same reduction.  Cause not found yet.")


@pytest.mark.parametrize("first", ["model 1", pytest.param("model 2", marks=pytest.mark.xfail(strict=True, reason=_STALE_MEAN))])
def test_a_training_step_of_one_model_keeps_the_accumulating_gradients_of_another(first, monkeypatch):
    """two models with a segment each: model 1 steps through train_step.backward_and_step (which declares ITS gradients consumed), model 2
    accumulates across that step; the step itself parks nothing.  first: whose segment is captured first"""
    from sparse2dense_amd import graphed
    from sparse2dense_amd.solver import build_one_cycle_optimizer
    from sparse2dense_amd.train_step import backward_and_step

    def body(toys):
        one, two = toys
        opt = build_one_cycle_optimizer(one.net, dict(wd=0.01))
        if first == "model 1":
            one.capture("A0")
        s = {mb: two.capture(mb) for mb in ("A0", "B0")}
        s["A1"] = two.single("A1")
        if first == "model 2":
            one.capture("A0")
        out = {}
        for p in two.params:
            p.grad = None
        two.loss("A0").backward()
        loss = one.loss("A1")   # (this replay parks the gradients model 1's capture left bound: nobody declared them consumed)
        parked = graphed.stats["parked"]
        backward_and_step(loss, one.params, opt, None, 0, 35.0)
        one.loss("A0")   # (model 1's next forward: a training step's gradients are not parked)
        assert graphed.stats["parked"] == parked, graphed.stats
        two.loss("B0").backward()
        two.loss("A1").backward()
        out["model 2 across model 1's step"] = (_grads(two.params), [s["A0"], s["B0"], s["A1"]])
        out["model 1's stepped weights"] = ([p.detach().clone() for p in one.params], [[p.detach().clone() for p in one.params]])
        return out
    _toy_compare(body, monkeypatch, n_models=2)


def test_a_discarded_forward_then_a_normal_step(monkeypatch):
    """a grad-mode forward whose outputs are dropped without a backward: the next calls replay (nothing stays pending) and give the right
    gradients"""
    def body(toys):
        toy = toys[0]
        s = {"A0": toy.capture("A0"), "A1": toy.single("A1")}
        toy.loss("A1")   # dropped
        out = {"after a discarded forward": (toy.single("A0"), [s["A0"]])}
        toy.loss("A0")   # dropped again, then accumulation
        out["accumulated after it"] = (_accumulate(toy, "A1", "A0"), [s["A1"], s["A0"]])
        return out
    st = _toy_compare(body, monkeypatch)
    assert st["replay"] == 7 and st["eager"] == 2, st


def test_capture_eviction_is_least_recently_used(monkeypatch):
    """MAX_CAPTURES = 2; hot, cold1, hot, cold2, hot: the capture in use is never the one dropped"""
    from sparse2dense_amd import dense2d, graphed, side
    monkeypatch.setattr(graphed, "MAX_CAPTURES", 2)
    side.enable(False)
    dense2d.clear_pack_cache()
    for k in graphed.stats:
        graphed.stats[k] = 0
    try:
        toy = _Toy()
        with torch.no_grad():
            for mb, n in (("A0", 3), ("B0", 3), ("A0", 1), ("C0", 3), ("A0", 1)):
                for _ in range(n):
                    toy.loss(mb)
        torch.cuda.synchronize()
    finally:
        dense2d.clear_pack_cache()
    st = graphed.stats
    assert st["capture"] == 3 and st["dropped"] == 1 and st["replay"] == 5 and st["eager"] == 6, st   # the last hot call replays
    assert {k: st[k] for k in ("eager", "capture", "replay", "dropped")} == _protocol(toy.calls, 2)


def _s2d_accumulation(graph):
    """the S2D student at 12 k points, micro-batches of B = 2 (two clouds) and B = 1 frames: the evaluation segment captured first, then the
    training captures of both batch sizes; then accumulation in both orders (pattern 1), two forwards before one backward (pattern 3) and
    an evaluation call between two accumulated backwards (pattern 4: at this level the evaluation runs through a segment of its own, with
    its own memory pool - the same-segment case is the toy-level test)"""
    from sparse2dense_amd import dense2d, graphed, hip_ops, side
    from sparse2dense_amd.data import SyntheticFrames
    side.enable(False)
    side.graph_defer("dense,aux,pcr")
    dense2d.clear_pack_cache()
    hip_ops.set_sparse_compute_dtype("s16")
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    model = _model("s2d_student", dev).train()
    if graph:
        model.use_hip_graphs()
    sets = {"2a": SyntheticFrames(2, n_points=12000, seed=5, distill=True, device=dev),
            "1": SyntheticFrames(1, n_points=12000, seed=15, distill=True, device=dev),
            "2b": SyntheticFrames(2, n_points=12000, seed=25, distill=True, device=dev)}
    params = [p for p in model.parameters() if p.requires_grad]
    for k in graphed.stats:
        graphed.stats[k] = 0
    calls, evals, trains = [], [], []

    def loss_of(k, conflict=False):
        calls.append((("train", k[0]), conflict))
        out = model(sets[k].example(), return_loss=True, return_feature=True)
        loss = sum(out[0]["loss"]) + out[4] + out[5]
        # every training call's loss terms and outputs, read at once (outputs are static buffers: valid until the segment's next call)
        trains.append([loss.detach().clone(), out[4].detach().clone(), out[5].detach().clone()] + [t.detach().clone() for t in out[0]["loss"]]
                      + [out[1].detach().float().clone(), out[2].detach().float().clone()]
                      + [v.detach().float().clone() for pr in out[3] for v in pr.values() if torch.is_tensor(v)])
        return loss

    def evaluate():
        calls.append((("eval",), False))
        model.eval()
        with torch.no_grad():
            out = model(sets["2b"].example(), return_loss=True, return_feature=True)
            evals.append((out[1].float().clone(), out[2].float().clone()))
        model.train()

    def single(k):
        for p in params:
            p.grad = None
        loss_of(k).backward()
        return _grads(params)
    res = {}
    try:
        for _ in range(3):
            evaluate()
        s = {}
        for k in ("2a", "1"):
            runs = [single(k) for _ in range(3)]   # warm-up calls + capture
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(runs[0], runs[2])), ("eager warm-up vs replay", k)
            s[k] = runs[2]
        s["2b"] = single("2b")
        for order in (("1", "2a"), ("2a", "1")):
            for p in params:
                p.grad = None
            for k in order:
                loss_of(k).backward()
            res["accumulated " + "+".join(order)] = (_grads(params), [s[k] for k in order])
        for p in params:            # zero_grad(set_to_none=False)
            if p.grad is not None:
                p.grad.zero_()
        loss_of("1").backward()
        loss_of("2a").backward()
        res["zeroed in place, accumulated 1+2a"] = (_grads(params), [s["1"], s["2a"]])
        for pair in (("2a", "2b"), ("2a", "1")):
            for p in params:
                p.grad = None
            (loss_of(pair[0]) + loss_of(pair[1], conflict=True)).backward()
            res["summed " + "+".join(pair)] = (_grads(params), [s[k] for k in pair])
        for p in params:
            p.grad = None
        loss_of("1").backward()
        evaluate()
        loss_of("2a").backward()
        res["1, evaluation, 2a"] = (_grads(params), [s["1"], s["2a"]])
        st = dict(graphed.stats)
    finally:
        hip_ops.set_sparse_compute_dtype("f32")
        dense2d.clear_pack_cache()
    return res, evals, trains, calls, st, [n for n, p in model.named_parameters() if p.requires_grad]


def test_s2d_student_accumulation_over_batch_sizes_two_forwards_and_evaluation_calls():
    """(the evaluation calls go through a segment of their own - another GraphedSegment, another memory pool - at this level; a forward-only
    replay of the SAME segment between backwards is test_forward_only_calls_between_backwards_and_before_the_optimizer_read)"""
    got, got_evals, got_trains, calls, st, names = _s2d_accumulation(True)
    ref, ref_evals, ref_trains, _, st0, _ = _s2d_accumulation(False)
    assert len(got_trains) == len(ref_trains) == len(calls) - 4
    for k, (a, b) in enumerate(zip(got_trains, ref_trains)):
        assert len(a) == len(b)
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), ("training call", k, "loss term / output", i)
    for what in got:
        for gs, rs in zip(got[what][1], ref[what][1]):
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(gs, rs)), (what, "single pass")
        _check_sums(what, got[what][0], ref[what][0], got[what][1], names)
    for k, ((a1, b1), (a0, b0)) in enumerate(zip(got_evals, ref_evals)):
        assert torch.equal(a1, a0) and torch.equal(b1, b0), f"evaluation call {k} differs from the kernel-by-kernel run"
    assert st0["replay"] == 0 and st["replay"] > 0, (st0, st)
    assert {k: st[k] for k in ("eager", "capture", "replay", "dropped")} == _protocol(calls), (st, _protocol(calls))
    assert st["capture"] == 3, st   # evaluation, B = 2, B = 1
