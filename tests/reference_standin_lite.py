"""Stand-ins for the reference's ``car.lite.config``, ``people.fhd.config`` and KITTI ``all.fhd.config`` networks on machines without the
reference checkout.

Same idea as tests/reference_standin.py, whose recipe this file reuses by import (``with_defaults``, ``build_voxelnet``): the object
is assembled through the public ``spconv`` / torch API the way the reference's constructors do it, and only the two sub-modules
that differ from car.fhd are replaced:

  * ``SimpleVoxelRadius`` (voxel_encoder.py:228-255): mean of the point slots, then ``[norm(mean[:, :2]), mean[:, 2:]]`` -- the torch
    formulation, three output channels, whatever the device (the module graph of this object is the baseline the fused path is
    compared with, so it must not call the fused path's kernel);
  * ``SpMiddleFHDLite`` (middle.py:418-483: four strided convs, paddings 1, 1, [0, 1, 1], 0) and ``SpMiddleFHDPeople``
    (middle.py:213-300: SpMiddleFHD minus one stride-2 level, paddings 1, [0, 1, 1], 0 on the strided layers).

tests/test_dropin_reference_lite.py (build container) checks type names, state-dict keys / shapes and ``dropin.model_config``
against the real ``build_network`` result.
"""
import numpy as np
import torch
from torch import nn

from reference_standin import build_middle as build_middle_fhd, build_voxelnet, with_defaults


def build_vfe(name, num_input_features):
    if name == "SimpleVoxelRadius":
        class SimpleVoxelRadius(nn.Module):
            def __init__(self):
                super().__init__()
                self.name, self.num_input_features = "SimpleVoxelRadius", num_input_features

            def forward(self, features, num_voxels, coors=None):
                mean = features[:, :, :self.num_input_features].sum(dim=1, keepdim=False) / num_voxels.type_as(features).view(-1, 1)
                return torch.cat([torch.norm(mean[:, :2], p=2, dim=1, keepdim=True), mean[:, 2:self.num_input_features]], dim=1)
        return SimpleVoxelRadius()

    class SimpleVoxel(nn.Module):
        def __init__(self):
            super().__init__()
            self.name, self.num_input_features = "SimpleVoxel", num_input_features

        def forward(self, features, num_voxels, coors=None):
            return (features[:, :, :self.num_input_features].sum(dim=1, keepdim=False) / num_voxels.type_as(features).view(-1, 1)).contiguous()
    return SimpleVoxel()


def build_middle(name, output_shape, num_input_features):
    import spconv
    BatchNorm1d = with_defaults(eps=1e-3, momentum=0.01)(nn.BatchNorm1d)
    SpConv3d = with_defaults(bias=False)(spconv.SparseConv3d)
    SubMConv3d = with_defaults(bias=False)(spconv.SubMConv3d)
    layers = []

    def add(conv, c):
        layers.extend([conv, BatchNorm1d(c), nn.ReLU()])
    if name == "SpMiddleFHDLite":
        add(SpConv3d(num_input_features, 16, 3, 2, padding=1), 16)
        add(SpConv3d(16, 32, 3, 2, padding=1), 32)
        add(SpConv3d(32, 64, 3, 2, padding=[0, 1, 1]), 64)
        add(SpConv3d(64, 64, (3, 1, 1), (2, 1, 1)), 64)
    else:
        assert name == "SpMiddleFHDPeople", name
        add(SubMConv3d(num_input_features, 16, 3, indice_key="subm0"), 16)
        add(SubMConv3d(16, 16, 3, indice_key="subm0"), 16)
        add(SpConv3d(16, 32, 3, 2, padding=1), 32)
        add(SubMConv3d(32, 32, 3, indice_key="subm1"), 32)
        add(SubMConv3d(32, 32, 3, indice_key="subm1"), 32)
        add(SpConv3d(32, 64, 3, 2, padding=[0, 1, 1]), 64)
        for _ in range(3):
            add(SubMConv3d(64, 64, 3, indice_key="subm2"), 64)
        add(SpConv3d(64, 64, (3, 1, 1), (2, 1, 1)), 64)

    class Middle(nn.Module):
        def __init__(self):
            super().__init__()
            self.name = name
            self.sparse_shape = np.array(output_shape[1:4]) + [1, 0, 0]
            self.middle_conv = spconv.SparseSequential(*layers)

        def forward(self, voxel_features, coors, batch_size):
            coors = coors.int()
            ret = spconv.SparseConvTensor(voxel_features, coors, self.sparse_shape, batch_size)
            ret = self.middle_conv(ret)
            ret = ret.dense()
            n, c, d, h, w = ret.shape
            return ret.view(n, c * d, h, w)
    return type(name, (Middle,), {})()


def build_voxelnet_lite(cfg):
    """``cfg``: second_amd.models.CAR_LITE, PEOPLE_FHD or ALL_FHD_KITTI (or a variation of one)."""
    net = build_voxelnet(cfg)
    gs = net.grid_size
    net.voxel_feature_extractor = build_vfe(cfg.get("vfe", "SimpleVoxel"), cfg["num_point_features"])
    if cfg["middle"] == "SpMiddleFHD":              # KITTI all.fhd.config: car.fhd's middle with three input channels
        net.middle_feature_extractor = build_middle_fhd([1] + gs[::-1].tolist() + [64], cfg["middle_in"])
    else:
        net.middle_feature_extractor = build_middle(cfg["middle"], [1] + gs[::-1].tolist() + [64], cfg["middle_in"])
    return net
