"""PIN (test infrastructure only) - builds the REFERENCE's own CPU rotated-IoU (det3d/ops/iou3d_nms/src/iou3d_cpu.cpp) into
oracle/_ref/ and calls it.  The source is compiled where it lies (read-only) together with oracle/ref_iou3d_bind.cpp; its two CUDA
includes are satisfied by empty stub headers written into oracle/_ref/stubs and its `__device__` qualifiers are defined away.
g++ -O2 -ffp-contract=off, the flags of the C oracle (oracle/Makefile).  tests/golden/make_golden_iou.py records what the binary
returns; tests/test_iou_pin.py holds oracle/iou_nms.c to it bit for bit."""
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("S2D_REFERENCE", "/root/reference")
SOURCE = os.path.join(REF, "det3d", "ops", "iou3d_nms", "src", "iou3d_cpu.cpp")
BIND = os.path.join(_HERE, "ref_iou3d_bind.cpp")
OUT = os.path.join(_HERE, "_ref")
NAME = "s2d_ref_iou3d"
_MOD = None


def reference_present():
    return os.path.isfile(SOURCE)


def built():
    return os.path.isfile(os.path.join(OUT, NAME + ".so"))


def _stamp():
    return "\n".join(f"{p} {os.stat(p).st_mtime_ns}" for p in (SOURCE, BIND, os.path.abspath(__file__)))


def build(verbose=False):
    """Compile the reference source + our binding into oracle/_ref/s2d_ref_iou3d.so; a no-op while the sources' mtimes are unchanged."""
    so, stamp_file = os.path.join(OUT, NAME + ".so"), os.path.join(OUT, NAME + ".stamp")
    if not reference_present():
        raise FileNotFoundError(f"reference source not found: {SOURCE}")
    stamp = _stamp()
    if os.path.isfile(so) and os.path.isfile(stamp_file) and open(stamp_file).read() == stamp:
        return so
    stubs = os.path.join(OUT, "stubs")
    os.makedirs(stubs, exist_ok=True)
    for header in ("cuda.h", "cuda_runtime_api.h"):
        with open(os.path.join(stubs, header), "w") as f:
            f.write("/* empty stub: the CPU source includes this header and uses nothing of it */\n")
    from torch.utils import cpp_extension
    cpp_extension.load(name=NAME, sources=[SOURCE, BIND], extra_include_paths=[stubs], build_directory=OUT, verbose=verbose,
                       extra_cflags=["-O2", "-ffp-contract=off", "-fno-fast-math", "-D__device__=", "-w"], is_python_module=False)
    with open(stamp_file, "w") as f:
        f.write(stamp)
    return so


def _module():
    global _MOD
    if _MOD is None:
        if not built():
            build()
        import torch  # noqa: F401  (libtorch must be loaded before the extension)
        spec = importlib.util.spec_from_file_location(NAME, os.path.join(OUT, NAME + ".so"))
        _MOD = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_MOD)
        sys.modules[NAME] = _MOD
    return _MOD


def boxes_iou_bev(a, b):
    """the reference binary's boxes_iou_bev_cpu of pcdet rows a [N, 7], b [M, 7]: float32 [N, M]"""
    import torch
    a = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    b = torch.from_numpy(np.ascontiguousarray(b, np.float32))
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32)
    if a.shape[0] and b.shape[0]:
        _module().boxes_iou_bev_cpu(a, b, out)
    return out.numpy()
