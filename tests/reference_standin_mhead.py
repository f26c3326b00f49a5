"""Stand-in for the reference's ``nuscenes/all.pp.mhead.config`` network (VoxelNetNuscenesMultiHead) on machines without the
reference checkout.

Same recipe as tests/reference_standin_lite.py: the object of tests/reference_standin.py with the sub-modules that differ replaced by
torch formulations under the reference's class names, attribute names and state-dict keys:

  * ``PillarFeatureNetRadius`` (pointpillars.py:240-325): decorations, padding mask, Linear(8, 64) + BatchNorm1d(eps 1e-3) + ReLU,
    max over the points -- torch only, whatever the device (this object's module graph is the baseline the fused path is compared
    with, so it must not call the fused path's kernel);
  * ``RPNNoHead`` (rpn.py:202-331, 500-529) returning ``stage<i>`` / ``up<i>`` / ``out``;
  * ``small_head`` (SmallObjectHead: three 3x3 convs whose norms are torch's DEFAULT BatchNorm2d -- eps 1e-5) and ``large_head``
    (DefaultHead) at top level, and ``network_forward`` as net_multi_head.py:150-176 has it: crop of ``round(0.1 * H)`` cells taken
    from stage 0's height, predictions concatenated large first.

tests/test_dropin_reference_mhead.py (build container) pins type names, state-dict keys / shapes and ``dropin.model_config`` to the
real ``build_network`` result.
"""
import numpy as np
import torch
from torch import nn

from reference_standin import build_voxelnet

SMALL = ["pedestrian", "traffic_cone", "bicycle", "motorcycle", "barrier"]
LARGE = ["car", "truck", "trailer", "bus", "construction_vehicle"]
CLASSES = ["bus", "car", "construction_vehicle", "trailer", "truck", "barrier", "bicycle", "motorcycle", "pedestrian", "traffic_cone"]


class PFNLayer(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.linear = nn.Linear(cin, cout, bias=False)
        self.norm = nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01)

    def forward(self, x):
        x = self.linear(x)
        x = torch.relu(self.norm(x.permute(0, 2, 1).contiguous()).permute(0, 2, 1).contiguous())
        return torch.max(x, dim=1, keepdim=True)[0]


class PillarFeatureNetRadius(nn.Module):
    def __init__(self, num_input_features, num_filters, voxel_size, pc_range):
        super().__init__()
        self.name, self._with_distance = "PillarFeatureNetRadius", False
        self.pfn_layers = nn.ModuleList([PFNLayer(num_input_features + 4, num_filters[0])])
        self.vx, self.vy = voxel_size[0], voxel_size[1]
        self.x_offset, self.y_offset = self.vx / 2 + pc_range[0], self.vy / 2 + pc_range[1]

    def forward(self, features, num_voxels, coors):
        dtype = features.dtype
        mean = features[:, :, :3].sum(dim=1, keepdim=True) / num_voxels.type_as(features).view(-1, 1, 1)
        f_cluster = features[:, :, :3] - mean
        f_center = torch.zeros_like(features[:, :, :2])
        f_center[:, :, 0] = features[:, :, 0] - (coors[:, 3].to(dtype).unsqueeze(1) * self.vx + self.x_offset)
        f_center[:, :, 1] = features[:, :, 1] - (coors[:, 2].to(dtype).unsqueeze(1) * self.vy + self.y_offset)
        radius = torch.norm(features[:, :, :2], p=2, dim=2, keepdim=True)
        dec = torch.cat([radius, features[:, :, 2:], f_cluster, f_center], dim=-1)
        t = dec.shape[1]
        mask = (torch.arange(t, device=dec.device).view(1, -1) < num_voxels.int().view(-1, 1)).type_as(dec).unsqueeze(-1)
        return self.pfn_layers[0](dec * mask).squeeze(1)


def build_voxelnet_mhead(cfg):
    """``cfg``: second_amd.models.ALL_PP_MHEAD (or a variation of it)."""
    net = build_voxelnet(cfg)
    assert type(net.rpn).__name__ == "RPNNoHead" and type(net.small_head).__name__ == "SmallObjectHead"
    assert all(m.eps == 1e-5 for m in net.small_head.net if isinstance(m, nn.BatchNorm2d))
    net.voxel_feature_extractor = PillarFeatureNetRadius(cfg["num_point_features"], cfg["vfe_filters"], cfg["voxel_size"],
                                                         cfg["point_cloud_range"])
    net.small_classes, net.large_classes = list(SMALL), list(LARGE)
    net.target_assigner.classes = list(CLASSES)
    net.target_assigner._feature_map_sizes = [list(f) for f in cfg["group_feature_map_sizes"]]

    def network_forward(self, voxels, num_points, coors, batch_size):
        voxel_features = self.voxel_feature_extractor(voxels, num_points, coors)
        spatial_features = self.middle_feature_extractor(voxel_features, coors, batch_size)
        rpn_out = self.rpn(spatial_features)
        r1 = rpn_out["stage0"]
        c = int(np.round(r1.shape[2] * 0.1))
        small = self.small_head(r1[:, :, c:-c, c:-c])
        large = self.large_head(rpn_out["out"])
        return {k: torch.cat([large[k], small[k]], dim=1) for k in large}
    net.__class__ = type("VoxelNetNuscenesMultiHead", (net.__class__,), {"network_forward": network_forward})
    net.name = "voxelnet"
    return net


def module_graph_dense(net, x):
    """The dense part of the stand-in's module graph on a pseudo image ``x`` [B, 64, H, W]: per-head prediction tensors
    ([B, A * H * W, code], large head first), as ``network_forward`` computes them before concatenating."""
    rpn_out = net.rpn(x)
    r1 = rpn_out["stage0"]
    c = int(np.round(r1.shape[2] * 0.1))
    return net.large_head(rpn_out["out"]), net.small_head(r1[:, :, c:-c, c:-c])
