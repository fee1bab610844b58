// PIN (test infrastructure only) - python binding of the reference's own CPU rotated-IoU entry point.  oracle/ref_iou3d.py compiles
// this file together with the reference's det3d/ops/iou3d_nms/src/iou3d_cpu.cpp, read where it lies; nothing of that file is copied here.
#include <torch/extension.h>

int boxes_iou_bev_cpu(at::Tensor boxes_a_tensor, at::Tensor boxes_b_tensor, at::Tensor ans_iou_tensor);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("boxes_iou_bev_cpu", &boxes_iou_bev_cpu, "reference BEV IoU of contiguous fp32 [N, 7] x [M, 7] pcdet boxes into [N, M]");
}
