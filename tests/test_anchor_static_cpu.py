"""Host side of the static anchor predict path (anchor_predict.StaticAnchorPlan, MultiGroupHead.predict_static): what it refuses - before
any HIP call, so all of it runs without a GPU - its sizes, its plan keys, and the C boundary of s2d_anchor_predict_finish_static."""
import copy
import os
import re

import pytest
import torch

from sparse2dense_amd import _lib, anchor_predict as AP, waymo_configs as WC
from sparse2dense_amd.registry import build_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = WC.SECOND_TEST_CFG
ENTRY = "s2d_anchor_predict_finish_static"


class _FakeCuda:
    """a tensor that says it lies on the device: lets the refusals behind the CPU check be reached without a GPU.  Only the host-side
    properties the checks read are answered; anything else is an error."""

    def __init__(self, t, device="cuda:0", ptr=4096):
        self._t, self.device, self._ptr = t, torch.device(device), ptr
        self.is_cuda, self.dtype, self.shape = True, t.dtype, t.shape

    def is_contiguous(self):
        return self._t.is_contiguous()

    def dim(self):
        return self._t.dim()

    def numel(self):
        return self._t.numel()

    def data_ptr(self):
        return self._ptr


@pytest.fixture
def no_hip(monkeypatch):
    """a refusal must come before the library is even loaded"""
    def load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", load)
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _FakeCuda)))


def _cfg(**nms):
    cfg = copy.deepcopy(CFG)
    cfg["nms"].update(nms)
    return cfg


def _table(a=12, device="cuda:0", ptr=4096, dtype=torch.float32):
    return _FakeCuda(torch.zeros((a, 7), dtype=dtype), device, ptr)


def _plan(cfg=CFG, classes=(3,), anchors=None, samples=2, use_direction=True, offset=0.0, device="cuda:0"):
    return AP.StaticAnchorPlan(cfg, list(classes), [_table()] * len(classes) if anchors is None else anchors, samples, use_direction, offset, device)


def test_the_plan_refuses_what_it_cannot_hold(no_hip):
    for pre_max, text in ((None, "nms_pre_max_size None"), (0, "nms_pre_max_size 0"), (4097, "nms_pre_max_size 4097"), (-3, "nms_pre_max_size -3")):
        with pytest.raises(_lib.S2DError, match=text):
            _plan(_cfg(nms_pre_max_size=pre_max))
    with pytest.raises(_lib.S2DError, match="9 tasks"):
        _plan(classes=[1] * 9)
    with pytest.raises(_lib.S2DError, match="CUDA device expected"):
        _plan(device="cpu")
    with pytest.raises(_lib.S2DError, match="1 anchor tables for 2 tasks"):
        _plan(classes=(1, 2), anchors=[_table()])
    with pytest.raises(_lib.S2DError, match="0 samples"):
        _plan(samples=0)
    with pytest.raises(_lib.S2DError, match="anchor table 0: a contiguous fp32"):
        _plan(anchors=[_table(dtype=torch.float64)])
    with pytest.raises(_lib.S2DError, match="anchor table 1: a contiguous fp32"):
        _plan(classes=(1, 1), anchors=[_table(), _FakeCuda(torch.zeros((12, 14))[:, ::2])])
    with pytest.raises(_lib.S2DError, match="anchor table 0: a contiguous fp32"):
        _plan(anchors=[_FakeCuda(torch.zeros((12, 8)))])
    with pytest.raises(_lib.S2DError, match="anchor table 0 is on cuda:1, the plan is built for cuda:0"):
        _plan(anchors=[_table(device="cuda:1")])


def _preds(b=2, a=12, classes=3):
    return [dict(box_preds=_FakeCuda(torch.zeros((b, a * 7))), cls_preds=_FakeCuda(torch.zeros((b, a * classes))),
                 dir_cls_preds=_FakeCuda(torch.zeros((b, a * 2))))]


def _head(cfg=None):
    return build_head(cfg or WC.second_voxelnet_train()["bbox_head"]).eval()


def test_predict_static_refuses_inputs_it_would_have_to_copy_or_widen(no_hip):
    head = _head()
    example = dict(anchors=[_table()])
    cpu = _preds()
    cpu[0]["cls_preds"] = torch.zeros((2, 36))
    with pytest.raises(_lib.S2DError, match="CUDA tensors expected.*'cls_preds'"):
        head.predict_static(example, cpu, CFG)
    with pytest.raises(_lib.S2DError, match="CUDA tensors expected.*'anchors'"):
        head.predict_static(dict(anchors=[torch.zeros((12, 7))]), _preds(), CFG)
    bf16 = _preds()
    bf16[0]["box_preds"] = _FakeCuda(torch.zeros((2, 84), dtype=torch.bfloat16))
    with pytest.raises(_lib.S2DError, match="'box_preds' is torch.bfloat16: fp32 only"):
        head.predict_static(example, bf16, CFG)
    strided = _preds()
    strided[0]["dir_cls_preds"] = _FakeCuda(torch.zeros((2, 48))[:, ::2])
    with pytest.raises(_lib.S2DError, match="'dir_cls_preds' is not contiguous"):
        head.predict_static(example, strided, CFG)
    with pytest.raises(_lib.S2DError, match="'anchors' is torch.float64"):
        head.predict_static(dict(anchors=[_table(dtype=torch.float64)]), _preds(), CFG)
    with pytest.raises(_lib.S2DError, match="'anchors' is not contiguous"):
        head.predict_static(dict(anchors=[_FakeCuda(torch.zeros((12, 14))[:, ::2])]), _preds(), CFG)
    missing = _preds()
    del missing[0]["dir_cls_preds"]
    assert head.use_direction_classifier
    with pytest.raises(_lib.S2DError, match="task 0 has no dir_cls_preds"):
        head.predict_static(example, missing, CFG)
    with pytest.raises(_lib.S2DError, match="9 tasks"):
        head.predict_static(dict(anchors=[_table()] * 9), _preds() * 9, CFG)
    with pytest.raises(_lib.S2DError, match="0 tasks"):
        head.predict_static(example, [], CFG)
    # the plan's own refusals reach the caller through the head
    with pytest.raises(_lib.S2DError, match="nms_pre_max_size 5000"):
        head.predict_static(example, _preds(), _cfg(nms_pre_max_size=5000))
    with pytest.raises(_lib.S2DError, match="nms_pre_max_size None"):
        head.predict_static(example, _preds(), _cfg(nms_pre_max_size=None))
    assert head.static_predict_calls == 0 and head.predict_paths == {"device": 0, "torch": 0} and head._static_plans == {}


def test_run_refuses_shapes_and_devices_that_differ_from_the_plans(no_hip):
    """`run`'s checks, on a plan whose buffers were never allocated (a GPU would be needed): only the fields the checks read are set"""
    plan = AP.StaticAnchorPlan.__new__(AP.StaticAnchorPlan)
    plan.tasks, plan.samples, plan.use_direction, plan.device = 1, 2, True, torch.device("cuda:0")
    plan.anchors, plan.num_anchors, plan.classes, plan.label_bases = [_table()], [12], [3], [0]
    for bad, text in ((_preds(b=3), "the plan was built for 2 samples, 12 anchors, 3 classes"), (_preds(a=13), "the plan was built for 2 samples, 12 anchors"),
                      (_preds(classes=2), "12 anchors, 3 classes"), (_preds() * 2, "2 tasks, the plan was built for 1")):
        with pytest.raises(_lib.S2DError, match=text):
            plan.run(bad)
    other = _preds()
    other[0]["cls_preds"] = _FakeCuda(torch.zeros((2, 36)), "cuda:1")
    with pytest.raises(_lib.S2DError, match="on cuda:0"):
        plan.run(other)
    short = _preds()
    short[0]["dir_cls_preds"] = _FakeCuda(torch.zeros((2, 12)))
    with pytest.raises(_lib.S2DError, match="the plan was built for"):
        plan.run(short)
    missing = _preds()
    del missing[0]["dir_cls_preds"]
    with pytest.raises(_lib.S2DError, match="no dir_cls_preds"):
        plan.run(missing)
    wide = _preds()
    wide[0]["box_preds"] = _FakeCuda(torch.zeros((2, 84), dtype=torch.float16))
    with pytest.raises(_lib.S2DError, match="fp32 only"):
        plan.run(wide)


def test_predict_static_raises_what_predict_raises(no_hip):
    head = _head()
    example, preds = dict(anchors=[_table()]), _preds()

    def edit(section, key, value):
        c = copy.deepcopy(CFG)
        (c[section] if section else c)[key] = value
        return c
    for bad, text in ((edit("nms", "use_multi_class_nms", True), "MultiGroupHead.predict: test_cfg.nms.use_multi_class_nms=True is not supported"),
                      (edit("nms", "use_rotate_nms", False), "MultiGroupHead.predict: test_cfg.nms.use_rotate_nms=False is not supported"),
                      (edit(None, "score_threshold", 0.0), "MultiGroupHead.predict: test_cfg.score_threshold <= 0 is not supported")):
        with pytest.raises(NotImplementedError) as err:
            head.predict_static(example, preds, bad)
        assert str(err.value) == text
    with pytest.raises(NotImplementedError) as err:
        head.predict_static(dict(example, anchors_mask=[None]), preds, CFG)
    assert str(err.value) == "MultiGroupHead.predict: anchors_mask (pos_area_threshold >= 0) is not supported"
    with pytest.raises(NotImplementedError, match="the 'mode' keyword"):
        head.predict_static(example, preds, CFG, mode=True)
    with pytest.raises(_lib.S2DError, match="the example carries no 'anchors'"):
        head.predict_static({}, preds, CFG)
    bev = copy.deepcopy(WC.second_voxelnet_train()["bbox_head"])
    bev["mode"] = "bev"
    with pytest.raises(NotImplementedError) as err:
        _head(bev).predict_static(example, preds, CFG)
    assert str(err.value) == "MultiGroupHead.predict: mode='bev' is not supported"
    assert head.static_predict_calls == 0 and head._static_plans == {}


def test_plan_keys_tell_apart_what_a_plan_depends_on():
    t12, t12b, t14 = _table(12, ptr=4096), _table(12, ptr=8192), _table(14, ptr=4096)
    key = lambda cfg=CFG, classes=(3,), anchors=(t12,), samples=2, use_dir=True, offset=0.0, dev="cuda:0": AP.static_plan_key(
        cfg, classes, list(anchors), samples, use_dir, offset, dev)
    base = key()
    assert base == key(copy.deepcopy(CFG)) and hash(base) == hash(key())
    others = [key(dict(CFG, score_threshold=0.2)), key(dict(CFG, post_center_limit_range=[])), key(dict(CFG, post_center_limit_range=[-70, -80, -10.0, 80, 80, 10.0])),
              key(_cfg(nms_pre_max_size=999)), key(_cfg(nms_post_max_size=99)), key(_cfg(nms_post_max_size=None)), key(_cfg(nms_iou_threshold=0.02)),
              key(classes=(2,)), key(classes=(1, 2), anchors=(t12, t12)), key(anchors=(t12b,)), key(anchors=(t14,)), key(samples=3), key(use_dir=False),
              key(offset=0.5), key(dev="cuda:1")]
    assert len({base, *others}) == len(others) + 1
    assert key(dict(CFG, max_per_img=7)) == base   # what the plan does not read does not count


def test_sizes(no_hip):
    """k, max_keep, the segment count, the padded score row, total and cap of a plan, from the constructor's arithmetic: the allocation
    needs a GPU and is stopped at the library load, which comes behind every size"""
    #        nms values, class counts, anchors per task, samples -> (k, max_keep, segs, max_anchors, total, cap)
    cases = [(dict(), (3,), [12], 2, (1000, 100, 2, 12, 2000, 100)),
             (dict(nms_post_max_size=None), (3,), [12], 2, (1000, 1000, 2, 12, 2000, 1000)),
             (dict(nms_pre_max_size=16, nms_post_max_size=5), (3,), [210], 3, (16, 5, 3, 210, 48, 5)),
             (dict(nms_pre_max_size=7, nms_post_max_size=83), (1, 2), [128, 256], 2, (7, 7, 4, 256, 28, 14)),
             (dict(nms_pre_max_size=4096, nms_post_max_size=4096), (1,) * 8, [5, 9, 5, 5, 5, 5, 5, 5], 1, (4096, 4096, 8, 9, 32768, 32768))]
    for nms, classes, sizes, samples, want in cases:
        plan = AP.StaticAnchorPlan.__new__(AP.StaticAnchorPlan)
        with pytest.raises(AssertionError, match="the library was loaded"):
            plan.__init__(_cfg(**nms), list(classes), [_table(a) for a in sizes], samples, True, 0.0, "cuda:0")
        assert (plan.k, plan.max_keep, plan.segs, plan.max_anchors, plan.total, plan.cap) == want, (nms, classes)
        assert plan.label_bases == [sum(classes[:t]) for t in range(len(classes))] and plan.samples == samples


def test_header_and_binding_agree_on_the_entry():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s2d.h")).read(), flags=re.S)
    decls = {}
    for name in (ENTRY, "s2d_anchor_predict_finish"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert decl, name
        decls[name] = [" ".join(p.split()) for p in decl.group(1).split(",")]
    params = decls[ENTRY]
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    assert restype is _lib.ctypes.c_int and len(params) == len(argtypes) == 21, (len(params), len(argtypes))
    for p, a in zip(params, argtypes):
        if "*" in p or p.startswith("s2d_stream_t"):
            assert a is _lib.ctypes.c_void_p, p
        elif p.startswith("float"):
            assert a is _lib.ctypes.c_float, p
        else:
            assert a is (_lib.ctypes.c_int64 if p.startswith("int64_t") else _lib.ctypes.c_int), p
    # the same parameter list as the per-segment finish, but for the name of the count array
    assert [p.replace("out_counts", "out_count") for p in params] == decls["s2d_anchor_predict_finish"]
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES["s2d_anchor_predict_finish"]


def test_the_entry_refuses_bad_sizes_without_a_device():
    from sparse2dense_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, ENTRY)
    tasks = (_lib.AnchorPredictTask * 8)()
    one = _lib.ctypes.c_void_p(64)   # never dereferenced: every call below is refused, or returns, before a launch

    def call(table=tasks, num_tasks=2, samples=2, total=16, max_keep=4, ins=one, segs=one, outs=one, out_counts=one):
        return getattr(lib, ENTRY)(table, num_tasks, samples, ins, ins, ins, ins, ins, segs, segs, total, ins, segs, max_keep, 1, 0.0,
                                   outs, outs, outs, out_counts, None)
    for bad, word in ((dict(table=None), "null task table"), (dict(num_tasks=0), "0 tasks"), (dict(num_tasks=9), "9 tasks"),
                      (dict(samples=-1), "bad samples -1"), (dict(samples=32768), "bad samples 32768"), (dict(num_tasks=8, samples=8192), "bad samples"),
                      (dict(total=-1), "negative size"), (dict(max_keep=-1), "negative size"), (dict(segs=None), "null segment arrays"),
                      (dict(out_counts=None), "out_counts"), (dict(ins=None), "null input"), (dict(outs=None), "null output")):
        assert call(**bad) == -1 and word in _lib.last_error(), (bad, _lib.last_error())
    assert call(samples=0) == 0
    assert call(samples=0, ins=None, segs=None, outs=None, out_counts=None) == 0
