#!/usr/bin/env python
"""Generates dcn_head_keys.npz by IMPORTING the reference (read-only) in the build container:

    python tests/golden/make_golden_dcn.py

  dcn_head_keys.npz    the KEY NAMES AND SHAPES of the reference's own CenterHead(dcn_head=True).state_dict()
                       (det3d/models/bbox_heads/center_head.py:25-63,112-164,219-232) for the bbox_head arguments of
                       configs/nusc/voxelnet/nusc_centerpoint_voxelnet_0075voxel_dcn.py - nothing else (no values).

The reference's DeformConv is a compiled CUDA extension that cannot be built here; a minimal nn.Module with the one `weight`
parameter of det3d/ops/dcn/deform_conv.py:226-228 stands in for it (the head is only constructed, never run)."""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from make_golden import save  # noqa: E402


class _DeformConvStandIn(torch.nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=False):
        super().__init__()
        assert not bias
        k = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        self.weight = torch.nn.Parameter(torch.zeros(out_channels, in_channels // groups, *k))


def main():
    MG.install_reference_stubs()
    sys.modules["det3d.ops.dcn"].DeformConv = _DeformConvStandIn
    MG._ns("det3d.core.utils.circle_nms_jit", circle_nms=None)
    ch = importlib.import_module("det3d.models.bbox_heads.center_head")
    from sparse2dense_amd import det3d_shim
    cfg_path = os.path.join(MG.REF, "configs/nusc/voxelnet/nusc_centerpoint_voxelnet_0075voxel_dcn.py")
    MG._ns("det3d.utils.config_tool", get_downsample_factor=det3d_shim.get_downsample_factor)   # (imported by the config file)
    spec = importlib.util.spec_from_file_location("_nusc_dcn_cfg", cfg_path)
    cfg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cfg)
    args = dict(cfg.model["bbox_head"])
    assert args.pop("type") == "CenterHead" and args["dcn_head"] is True
    head = ch.CenterHead(**args)
    sd = head.state_dict()
    keys = np.array(list(sd.keys()))
    shapes = np.zeros((len(keys), 4), dtype=np.int64) - 1
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = list(v.shape)
    save("dcn_head_keys.npz", keys=keys, shapes=shapes)


if __name__ == "__main__":
    main()
