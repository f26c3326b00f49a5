"""Host-side mirror of the reference's VoxelNet forward for the configurations BASELINE.json names.

The GPU box has no /root/reference, so bench.py / smoke() / -m gpu tests cannot import the reference's
model code; this module restates the network *topology* (never the code) with the same module names,
parameter shapes and state_dict keys as second/pytorch/models/{voxelnet,middle,rpn,voxel_encoder}.py, so a
reference ``.tckpt`` loads into it and the unmodified reference model (running over our drop-in ``spconv``)
produces the same numbers (tests/test_dropin_reference.py checks that in the build container).

    SimpleVoxel      voxel_encoder.py:207-225   (fused into the voxeliser's epilogue on the native path)
    SpMiddleFHD      middle.py:111-210          (spconv.SubMConv3d / SparseConv3d stack)
    RPNV2            rpn.py:202-420,468-497     (inference: hand-written MFMA convs, sec_conv2d_nhwc / sec_conv1x1_chain_nhwc;
                                                 training and multi-block RPNs: torch convs)
    predict          voxelnet.py:377-645        (decode -> score filter -> top-k -> rotated NMS -> direction fix)
"""
import math
import os

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

import spconv
from . import ops


# ------------------------------------------------------------------------------------------ config
CAR_FHD = dict(
    name="car.fhd",
    point_cloud_range=[0, -40, -3, 70.4, 40, 1], voxel_size=[0.05, 0.05, 0.1], max_points_per_voxel=5,
    max_voxels=40000, num_point_features=4,
    middle="SpMiddleFHD", middle_in=4,
    rpn=dict(layer_nums=[5], layer_strides=[1], num_filters=[128], upsample_strides=[1],
             num_upsample_filters=[128], num_input_features=128),
    downsample_factor=8,
    anchor_sizes=[[1.6, 3.9, 1.56]], anchor_ranges=[[0, -40.0, -1.00, 70.4, 40.0, -1.00]], rotations=[0, 1.57],
    matched_thresholds=[0.6], unmatched_thresholds=[0.45], assign_per_class=True,
    num_class=1, num_direction_bins=2, direction_offset=0.0, direction_limit_offset=1.0,
    nms_score_threshold=0.3, nms_pre_max_size=1000, nms_post_max_size=100, nms_iou_threshold=0.01,
    use_rotate_nms=True, post_center_range=[0, -40, -2.2, 70.4, 40, 0.8],
)  # second/configs/car.fhd.config


ALL_PP_LARGEA = dict(
    name="nuscenes/all.pp.largea",
    point_cloud_range=[-50, -50, -10, 50, 50, 10], voxel_size=[0.25, 0.25, 20], max_points_per_voxel=60,
    max_voxels=30000, num_point_features=4,
    vfe="PillarFeatureNet", vfe_filters=[64], middle="PointPillarsScatter", middle_in=64,
    rpn=dict(layer_nums=[3, 5, 5], layer_strides=[2, 2, 2], num_filters=[64, 128, 256],
             upsample_strides=[0.25, 0.5, 1], num_upsample_filters=[128, 128, 128], num_input_features=64),
    downsample_factor=8,
    # anchored classes (car, bus, construction_vehicle, trailer x2 sizes, truck); the other five are `no_anchor`
    anchor_sizes=[[1.95017717, 4.60718145, 1.72270761], [2.94046906, 11.1885991, 3.47030982],
                  [2.73050468, 6.38352896, 3.13312415], [3, 15, 3.8], [2, 3, 3.8], [2.4560939, 6.73778078, 2.73004906]],
    anchor_ranges=[[-50, -50, -0.93897414, 50, 50, -0.93897414], [-50, -50, -0.0715754, 50, 50, -0.0715754],
                   [-50, -50, -0.08168083, 50, 50, -0.08168083], [-50, -50, 0.22228277, 50, 50, 0.22228277],
                   [-50, -50, 0.22228277, 50, 50, 0.22228277], [-50, -50, -0.37937912, 50, 50, -0.37937912]],
    anchor_groups=[[0], [1], [2], [3, 4], [5]],   # sizes belonging to one anchor generator (class)
    # class ids (1-based position in class_settings) of the anchored classes; assign_all with per-anchor thresholds (:269)
    group_class_ids=[1, 2, 3, 4, 5], matched_thresholds=[0.4, 0.5, 0.5, 0.5, 0.5],
    unmatched_thresholds=[0.3, 0.35, 0.35, 0.35, 0.35], assign_per_class=False,
    rotations=[0, 1.57],
    num_class=10, num_direction_bins=2, direction_offset=0.78, direction_limit_offset=0.0,
    nms_score_threshold=0.05, nms_pre_max_size=1000, nms_post_max_size=300, nms_iou_threshold=0.5,
    use_rotate_nms=False, post_center_range=[-59.6, -59.6, -10, 59.6, 59.6, 10],
)  # second/configs/nuscenes/all.pp.largea.config


ALL_FHD_NUSC = dict(
    name="nuscenes/all.fhd",
    point_cloud_range=[-49.6, -49.6, -5, 49.6, 49.6, 3], voxel_size=[0.05, 0.05, 0.2], max_points_per_voxel=1,
    max_voxels=90000, num_point_features=4,
    block_filtering=dict(block_factor=1, block_size=8, height_threshold=0.2),   # ground-block filter
    middle="SpMiddleFHD", middle_in=4,
    rpn=dict(layer_nums=[5], layer_strides=[1], num_filters=[128], upsample_strides=[0.5],   # 0.5 = stride-2 conv
             num_upsample_filters=[128], num_input_features=128),
    downsample_factor=16,
    # car, bicycle, bus, construction_vehicle, motorcycle, pedestrian, traffic_cone, trailer (2 sizes), truck, barrier
    anchor_sizes=[[1.95017719, 4.60718155, 1.72270763], [0.6005891, 1.68452156, 1.27192199],
                  [2.94046903, 11.18859863, 3.47030973], [2.73050475, 6.38352919, 3.13312411],
                  [0.76279479, 2.09973788, 1.44403028], [0.66344887, 0.72564369, 1.75748074],
                  [0.39694518, 0.40359262, 1.06232154], [3.0, 15.0, 3.8], [2.0, 3.0, 3.8],
                  [2.45609379, 6.73778057, 2.73004913], [2.49008846, 0.48578221, 0.98297065]],
    anchor_ranges=[[-49.6, -49.6, z, 49.6, 49.6, z] for z in
                   (-0.93897414, -1.03743017, -0.0715754, -0.08168083, -0.99194854, -0.73911035, -1.27868915,
                    0.22228277, 0.22228277, -0.37937912, -1.27247965)],
    anchor_groups=[[0], [1], [2], [3], [4], [5], [6], [7, 8], [9], [10]],
    rotations=[0, 1.57], group_rotations={5: [0], 6: [0]},   # pedestrian / traffic_cone: one rotation
    group_class_ids=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10], matched_thresholds=[0.4, 0.2, 0.5, 0.4, 0.2, 0.5, 0.5, 0.5, 0.5, 0.3],
    unmatched_thresholds=[0.3, 0.15, 0.35, 0.3, 0.15, 0.35, 0.35, 0.35, 0.35, 0.2], assign_per_class=True,   # :85-295
    num_class=10, num_direction_bins=2, direction_offset=0.78, direction_limit_offset=0.0,
    nms_score_threshold=0.05, nms_pre_max_size=1000, nms_post_max_size=300, nms_iou_threshold=0.5,
    use_rotate_nms=False, post_center_range=[-59.6, -59.6, -10, 59.6, 59.6, 10],
)  # second/configs/nuscenes/all.fhd.config

# The region_similarity_calculator of every anchor generator of all.fhd.config (:85-295): pedestrian and traffic_cone (groups 5, 6)
# get distance_similarity { distance_norm: 1.414, with_rotation: false, rotation_alpha: 0.0 }, every other class
# nearest_iou_similarity.  ALL_FHD_NUSC itself carries no ``group_similarity`` key and therefore matches those two classes by
# near-box IoU; dict(ALL_FHD_NUSC, group_similarity=NUSC_FHD_GROUP_SIMILARITY) is the reference's assignment.
NUSC_FHD_GROUP_SIMILARITY = [None if gi not in (5, 6) else dict(kind="distance", distance_norm=1.414, with_rotation=False,
                                                                rotation_alpha=0.0) for gi in range(10)]


CAR_LITE = dict(
    name="car.lite",
    point_cloud_range=[0, -32.0, -3, 52.8, 32.0, 1], voxel_size=[0.05, 0.05, 0.1], max_points_per_voxel=1,
    max_voxels=30000, num_point_features=4,
    vfe="SimpleVoxelRadius", middle="SpMiddleFHDLite", middle_in=3,
    rpn=dict(layer_nums=[5], layer_strides=[1], num_filters=[128], upsample_strides=[1],
             num_upsample_filters=[128], num_input_features=128),
    downsample_factor=8,
    anchor_sizes=[[1.6, 3.9, 1.56]], anchor_ranges=[[0, -32.0, -1.0, 52.8, 32.0, -1.0]], rotations=[0, 1.57],
    matched_thresholds=[0.6], unmatched_thresholds=[0.45], assign_per_class=True,
    num_class=1, num_direction_bins=2, direction_offset=0.0, direction_limit_offset=1.0,
    nms_score_threshold=0.3, nms_pre_max_size=1000, nms_post_max_size=100, nms_iou_threshold=0.01,
    use_rotate_nms=True, post_center_range=[0, -40, -2.2, 70.4, 40, 0.8],
)  # second/configs/car.lite.config ("SECOND lite": 160 x 132 feature map)


PEOPLE_FHD = dict(
    name="people.fhd",
    point_cloud_range=[0, -20, -2.5, 48, 20, 0.5], voxel_size=[0.05, 0.05, 0.15], max_points_per_voxel=5,
    max_voxels=40000, num_point_features=4,
    vfe="SimpleVoxel", middle="SpMiddleFHDPeople", middle_in=4,
    rpn=dict(layer_nums=[5], layer_strides=[1], num_filters=[128], upsample_strides=[1],
             num_upsample_filters=[128], num_input_features=128),
    downsample_factor=4,
    # Cyclist, Pedestrian
    anchor_sizes=[[0.6, 1.76, 1.73], [0.6, 0.8, 1.73]],
    anchor_ranges=[[0, -20, -0.6, 48, 20.0, -0.6], [0, -20, -0.6, 48, 20.0, -0.6]], rotations=[0, 1.57],
    matched_thresholds=[0.5, 0.5], unmatched_thresholds=[0.35, 0.35], assign_per_class=True,
    num_class=2, num_direction_bins=2, direction_offset=0.0, direction_limit_offset=1.0,
    nms_score_threshold=0.4, nms_pre_max_size=1000, nms_post_max_size=100, nms_iou_threshold=0.2,
    use_rotate_nms=True, post_center_range=[0, -20, -2.5, 48.4, 20, -0.5],
)  # second/configs/people.fhd.config (200 x 240 feature map)


ALL_FHD_KITTI = dict(
    name="all.fhd",
    point_cloud_range=[0, -32.0, -3, 52.8, 32.0, 1], voxel_size=[0.05, 0.05, 0.1], max_points_per_voxel=5,
    max_voxels=60000, num_point_features=4,
    vfe="SimpleVoxelRadius", middle="SpMiddleFHD", middle_in=3,
    rpn=dict(layer_nums=[5, 5], layer_strides=[1, 2], num_filters=[64, 128], upsample_strides=[1, 2],
             num_upsample_filters=[128, 128], num_input_features=128),
    downsample_factor=8,
    # Car, Cyclist, Pedestrian, Van
    anchor_sizes=[[1.6, 3.9, 1.56], [0.6, 1.76, 1.73], [0.6, 0.8, 1.73], [1.87103749, 5.02808195, 2.20964255]],
    anchor_ranges=[[0, -32.0, z, 52.8, 32.0, z] for z in (-1.0, -0.6, -0.6, -1.41)], rotations=[0, 1.57],
    matched_thresholds=[0.6, 0.35, 0.35, 0.6], unmatched_thresholds=[0.45, 0.2, 0.2, 0.45], assign_per_class=True,
    num_class=4, num_direction_bins=2, direction_offset=0.0, direction_limit_offset=1.0,
    nms_score_threshold=0.3, nms_pre_max_size=1000, nms_post_max_size=100, nms_iou_threshold=0.1,
    use_rotate_nms=True, post_center_range=[0, -40, -2.2, 70.4, 40, 0.8],
)  # second/configs/all.fhd.config (KITTI, four classes, two-block RPN, 160 x 132 feature map)


KITTI_PP_CAR_16 = dict(
    name="pointpillars/car/xyres_16",
    point_cloud_range=[0, -39.68, -3, 69.12, 39.68, 1], voxel_size=[0.16, 0.16, 4], max_points_per_voxel=100,
    max_voxels=12000, num_point_features=4,
    vfe="PillarFeatureNet", vfe_filters=[64], middle="PointPillarsScatter", middle_in=64,
    rpn=dict(layer_nums=[3, 5, 5], layer_strides=[2, 2, 2], num_filters=[64, 128, 256],
             upsample_strides=[1, 2, 4], num_upsample_filters=[128, 128, 128], num_input_features=64),
    downsample_factor=2,
    # anchor_generator_stride: centres = index * stride + offset in fp32 (box_np_ops.create_anchors_3d_stride), not a linspace over a range
    anchor_sizes=[[1.6, 3.9, 1.56]], anchor_strides=[[0.32, 0.32, 0.0]], anchor_offsets=[[0.16, -39.52, -1.78]], rotations=[0, 1.57],
    matched_thresholds=[0.6], unmatched_thresholds=[0.45], assign_per_class=True,
    num_class=1, num_direction_bins=2, direction_offset=0.0, direction_limit_offset=1.0,
    nms_score_threshold=0.05, nms_pre_max_size=1000, nms_post_max_size=300, nms_iou_threshold=0.5,
    use_rotate_nms=False, post_center_range=[0, -39.68, -5, 69.12, 39.68, 5],
    # both input readers set it: anchors over (nearly) empty ground are dropped before the score threshold of predict and pruned from
    # the target assignment (preprocess.py:345-357).  Absent or negative = no mask (every other config)
    anchor_area_threshold=1,
)  # second/configs/pointpillars/car/xyres_16.config (432 x 496 pillars, 216 x 248 feature map)


ALL_PP_MHEAD = dict(
    name="nuscenes/all.pp.mhead",
    point_cloud_range=[-50, -50, -5, 50, 50, 3], voxel_size=[0.25, 0.25, 8], max_points_per_voxel=60,
    max_voxels=30000, num_point_features=4,
    vfe="PillarFeatureNetRadius", vfe_filters=[64], middle="PointPillarsScatter", middle_in=64,
    # RPNNoHead (rpn.py:500-529): the trunk only; its heads are the network's (net_multi_head.py:121-176)
    rpn_class="RPNNoHead",
    rpn=dict(layer_nums=[3, 5, 5], layer_strides=[2, 2, 2], num_filters=[64, 128, 256],
             upsample_strides=[0.5, 1, 2], num_upsample_filters=[128, 128, 128], num_input_features=64,
             use_direction_classifier=True),
    downsample_factor=4,       # of the trunk's concatenated map (400 -> 100), the large head's
    # the two heads in prediction order (large first, then small): which map each reads, its anchors per cell, its anchor map.
    # small_head reads block 0's output (200 x 200) cropped by round(0.1 * 200) = 20 cells per side
    heads=[dict(name="large_head", source="out", num_anchor_per_loc=12, feature_map_size=[1, 100, 100]),
           dict(name="small_head", source="stage0", num_anchor_per_loc=8, feature_map_size=[1, 160, 160])],
    # bus, car, construction_vehicle, trailer (2 sizes), truck | barrier, bicycle, motorcycle, pedestrian, traffic_cone
    anchor_sizes=[[2.94046906, 11.1885991, 3.47030982], [1.95017717, 4.60718145, 1.72270761], [2.73050468, 6.38352896, 3.13312415],
                  [3, 15, 3.8], [2, 3, 3.8], [2.4560939, 6.73778078, 2.73004906],
                  [2.49008838, 0.48578221, 0.98297065], [0.60058911, 1.68452161, 1.27192197], [0.76279481, 2.09973778, 1.44403034],
                  [0.66344886, 0.7256437, 1.75748069], [0.39694519, 0.40359262, 1.06232151]],
    anchor_ranges=[[-50, -50, z, 50, 50, z] for z in (-0.0715754, -0.93897414, -0.08168083, 0.22228277, 0.22228277, -0.37937912)]
    + [[-40, -40, z, 40, 40, z] for z in (-1.27247968, -1.03743013, -0.99194854, -0.73911038, -1.27868911)],
    anchor_groups=[[0], [1], [2], [3, 4], [5], [6], [7], [8], [9], [10]],
    group_feature_map_sizes=[[1, 100, 100]] * 5 + [[1, 160, 160]] * 5,      # class_settings.feature_map_size (:94 ... :284)
    rotations=[0, 1.57], group_rotations={8: [0], 9: [0]},   # pedestrian / traffic_cone: one rotation
    group_class_ids=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10], matched_thresholds=[0.5, 0.4, 0.4, 0.5, 0.5, 0.3, 0.3, 0.3, 0.2, 0.5],
    unmatched_thresholds=[0.35, 0.3, 0.3, 0.35, 0.35, 0.2, 0.2, 0.2, 0.1, 0.35], assign_per_class=True,
    num_class=10, num_direction_bins=2, direction_offset=0.78, direction_limit_offset=0.0,
    nms_score_threshold=0.05, nms_pre_max_size=1000, nms_post_max_size=300, nms_iou_threshold=0.5,
    use_rotate_nms=False, post_center_range=[-59.6, -59.6, -10, 59.6, 59.6, 10],
)  # second/configs/nuscenes/all.pp.mhead.config (VoxelNetNuscenesMultiHead: 120 000 + 204 800 anchors)


ALL_PP_MIDA = dict(
    name="nuscenes/all.pp.mida",
    point_cloud_range=[-50, -50, -5, 50, 50, 3], voxel_size=[0.25, 0.25, 8], max_points_per_voxel=60,
    max_voxels=30000, num_point_features=4,
    # PillarFeatureNetOld: the centre offsets stand in the raw x, y columns too (models.PillarFeatureNetOld); with_distance: false
    vfe="PillarFeatureNetOld", vfe_filters=[64], vfe_with_distance=False, middle="PointPillarsScatter", middle_in=64,
    rpn=dict(layer_nums=[3, 5, 5], layer_strides=[2, 2, 2], num_filters=[64, 128, 256],
             upsample_strides=[0.5, 1, 2], num_upsample_filters=[128, 128, 128], num_input_features=64),
    downsample_factor=4,       # 400 x 400 pillars -> one 100 x 100 map, 20 anchors per cell
    # car, bicycle, bus, construction_vehicle, motorcycle, pedestrian, traffic_cone, trailer (2 sizes), truck, barrier
    anchor_sizes=[[1.95017717, 4.60718145, 1.72270761], [0.60058911, 1.68452161, 1.27192197], [2.94046906, 11.1885991, 3.47030982],
                  [2.73050468, 6.38352896, 3.13312415], [0.76279481, 2.09973778, 1.44403034], [0.66344886, 0.7256437, 1.75748069],
                  [0.39694519, 0.40359262, 1.06232151], [3, 15, 3.8], [2, 3, 3.8], [2.4560939, 6.73778078, 2.73004906],
                  [2.49008838, 0.48578221, 0.98297065]],
    anchor_ranges=[[-50, -50, z, 50, 50, z] for z in
                   (-0.93897414, -1.03743013, -0.0715754, -0.08168083, -0.99194854, -0.73911038, -1.27868911,
                    0.22228277, 0.22228277, -0.37937912, -1.27247968)],
    anchor_groups=[[0], [1], [2], [3], [4], [5], [6], [7, 8], [9], [10]],
    rotations=[0, 1.57], group_rotations={5: [0], 6: [0]},   # pedestrian / traffic_cone: one rotation
    group_class_ids=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10], matched_thresholds=[0.25, 0.2, 0.5, 0.4, 0.2, 0.5, 0.5, 0.5, 0.5, 0.3],
    unmatched_thresholds=[0.2, 0.15, 0.35, 0.3, 0.15, 0.35, 0.35, 0.35, 0.35, 0.2], assign_per_class=True,
    # pedestrian / traffic_cone: distance_similarity { distance_norm: 1.414, with_rotation: false, rotation_alpha: 0.0 }
    group_similarity=[None if gi not in (5, 6) else dict(kind="distance", distance_norm=1.414, with_rotation=False, rotation_alpha=0.0)
                      for gi in range(10)],
    num_class=10, num_direction_bins=2, direction_offset=0.0, direction_limit_offset=0.0,   # no direction_offset in the config
    nms_score_threshold=0.05, nms_pre_max_size=1000, nms_post_max_size=300, nms_iou_threshold=0.5,
    use_rotate_nms=False, post_center_range=[-59.6, -59.6, -10, 59.6, 59.6, 10],
)  # second/configs/nuscenes/all.pp.mida.config (VoxelNet, one head: 100 x 100 x 20 = 200 000 anchors)


def anchor_area_threshold_of(cfg):
    """The config's ``anchor_area_threshold`` when it asks for the anchor-area mask (>= 0), else None."""
    thr = cfg.get("anchor_area_threshold", -1)
    return float(thr) if thr is not None and thr >= 0 else None


def anchors_per_location(cfg):
    """target_assigner.num_anchors_per_location (target_assigner.py:249-254): sum over generators of sizes x rotations."""
    groups = cfg.get("anchor_groups") or [[i] for i in range(len(cfg["anchor_sizes"]))]
    return sum(len(g) * len(cfg.get("group_rotations", {}).get(gi, cfg["rotations"])) for gi, g in enumerate(groups))


def group_feature_map_size(cfg, gi, feature_map_size):
    """The anchor map of generator ``gi``: its own ``feature_map_size`` when the config gives one per class (class_settings.feature_map_size,
    target_assigner.py:179-189: the multi-head networks), else the network's."""
    sizes = cfg.get("group_feature_map_sizes")
    return [int(v) for v in (sizes[gi] if sizes and sizes[gi] else feature_map_size)]


def multiclass_nms_settings(cfg, a_per_loc, feature_map_size):
    """The per-class settings of ``multiclass_nms`` (the reference's use_multi_class_nms, voxelnet.py:458-547), or None without the key.
    Keys read: ``nms_class_agnostic`` and the per-class lists ``nms_score_thresholds``, ``nms_pre_max_sizes``, ``nms_post_max_sizes``,
    ``nms_iou_thresholds`` (each defaults to the scalar setting for every class); the classes' anchor ranges come from
    ``class_anchor_ranges`` ((begin, end) anchor indices per class: target_assigner.anchors_range) or, with an anchor table in the
    config, from :func:`anchor_class_ranges`.  -> dict(thr, pre, post, iou, agnostic, a_ranges [(a_begin, a_end)], post_offsets, P)."""
    if not cfg.get("multiclass_nms"):
        return None
    nc = int(cfg["num_class"])
    if cfg.get("heads"):
        raise ValueError(f"{cfg.get('name')}: multiclass_nms on a multi-head network is not supported")

    def per_class(key, scalar, conv):
        v = cfg.get(key)
        v = [cfg[scalar]] * nc if v is None else list(v)
        if len(v) != nc:
            raise ValueError(f"{cfg.get('name')}: {key} has {len(v)} entries for {nc} classes")
        return [conv(x) for x in v]
    thr = per_class("nms_score_thresholds", "nms_score_threshold", float)
    pre = per_class("nms_pre_max_sizes", "nms_pre_max_size", int)
    post = per_class("nms_post_max_sizes", "nms_post_max_size", int)
    iou = per_class("nms_iou_thresholds", "nms_iou_threshold", float)
    if min(thr) <= 0.0:
        raise ValueError(f"{cfg.get('name')}: multiclass_nms with a score threshold <= 0 is not supported")
    if min(pre) <= 0 or min(post) <= 0:
        raise ValueError(f"{cfg.get('name')}: multiclass_nms needs positive nms_pre_max_sizes / nms_post_max_sizes")
    agnostic = bool(cfg.get("nms_class_agnostic", False))
    hw = int(feature_map_size[1]) * int(feature_map_size[2])
    if agnostic:
        a_ranges = [(0, a_per_loc)] * nc
    else:
        rng = cfg.get("class_anchor_ranges")
        if rng is None:
            begin = anchor_class_ranges(cfg, feature_map_size)
            rng = list(zip(begin[:-1], begin[1:]))
        if len(rng) != nc or any(int(lo) % hw or int(hi) % hw or not 0 <= int(lo) < int(hi) <= a_per_loc * hw for lo, hi in rng):
            raise ValueError(f"{cfg.get('name')}: multiclass_nms needs one anchor range per class, each whole anchors-per-location "
                             f"planes of the {feature_map_size[1]} x {feature_map_size[2]} map, got {list(rng)}")
        a_ranges = [(int(lo) // hw, int(hi) // hw) for lo, hi in rng]
    offsets = [0]
    for p in post:
        offsets.append(offsets[-1] + p)
    return dict(thr=thr, pre=pre, post=post, iou=iou, agnostic=agnostic, a_ranges=a_ranges, post_offsets=offsets, P=offsets[-1], device={})


def anchor_class_ranges(cfg, feature_map_size):
    """Start of every anchor generator's range in the class-major anchor array of generate_anchors (+ the total)."""
    groups = cfg.get("anchor_groups") or [[i] for i in range(len(cfg["anchor_sizes"]))]
    begin = [0]
    for gi, g in enumerate(groups):
        d, h, w = group_feature_map_size(cfg, gi, feature_map_size)
        begin.append(begin[-1] + len(g) * len(cfg.get("group_rotations", {}).get(gi, cfg["rotations"])) * d * h * w)
    return begin


def grid_size_of(cfg):
    r = np.array(cfg["point_cloud_range"], np.float32)
    v = np.array(cfg["voxel_size"], np.float32)
    return np.round((r[3:] - r[:3]) / v).astype(np.int64)  # (x, y, z)


def anchor_custom_values(cfg, num_groups=None):
    """``cfg["anchor_custom_values"]`` -- the anchor generators' custom_values (second/core/anchor_generator.py:30-70; nuScenes:
    ``[0, 0]``, the velocity's base value) -- as one float32 array per anchor group.  The key holds a list of floats (every group's) or
    one such list per group, all of one length (the reference asserts equal ndim across generators, target_assigner.py:22-23); absent
    or empty: no custom values, [] * groups.  More than ops.BOX_MAX_NDIM - 7 values are refused."""
    v = cfg.get("anchor_custom_values")
    nested = v is not None and len(v) > 0 and isinstance(v[0], (list, tuple, np.ndarray))
    if num_groups is None:      # (a config adopted from a reference-built network has no anchor table: one list per generator it had)
        num_groups = len(cfg.get("anchor_groups") or cfg.get("anchor_sizes") or (v if nested else [0]))
    if v is None or len(v) == 0:
        return [np.zeros((0,), np.float32)] * num_groups
    per_group = [list(g) for g in v] if nested else [list(v)] * num_groups
    if len(per_group) != num_groups:
        raise ValueError(f"anchor_custom_values: {len(per_group)} lists for {num_groups} anchor groups")
    if len({len(g) for g in per_group}) != 1:
        raise ValueError(f"anchor_custom_values: every anchor group needs the same number of values, got {[len(g) for g in per_group]}")
    if len(per_group[0]) > ops.BOX_MAX_NDIM - 7:
        raise ValueError(f"anchor_custom_values: {len(per_group[0])} custom values; at most {ops.BOX_MAX_NDIM - 7} are supported "
                         f"(box rows of up to {ops.BOX_MAX_NDIM} values)")
    return [np.asarray(g, np.float64).astype(np.float32) for g in per_group]


def box_ndim_of(cfg):
    """Values per box row of a config: 7 + the number of custom values (GroundBox3dCoder.code_size, box_coders.py:31-46)."""
    return 7 + len(anchor_custom_values(cfg)[0])


def generate_anchors(cfg, feature_map_size):
    """[A*D*H*W, 7 + c] anchors ordered (anchor, z, y, x) like target_assigner.generate_anchors
    (second/core/target_assigner.py:169-207 over box_np_ops.create_anchors_3d_range :606-638); the c values of
    :func:`anchor_custom_values` are appended to every anchor of their group."""
    out = []
    groups = cfg.get("anchor_groups") or [[i] for i in range(len(cfg["anchor_sizes"]))]
    custom = anchor_custom_values(cfg, len(groups))
    for gi, grp in enumerate(groups):   # one anchor generator: (size, rotation) major, then z, y, x
        d, h, w = group_feature_map_size(cfg, gi, feature_map_size)
        rots = np.array(cfg.get("group_rotations", {}).get(gi, cfg["rotations"]), np.float32)
        if cfg.get("anchor_strides"):      # anchor_generator_stride (box_np_ops.create_anchors_3d_stride :561-604): fp32 index * stride + offset
            sx, sy, sz_ = cfg["anchor_strides"][grp[0]]
            ox, oy, oz = cfg["anchor_offsets"][grp[0]]
            zc = np.arange(d, dtype=np.float32) * sz_ + oz
            yc = np.arange(h, dtype=np.float32) * sy + oy
            xc = np.arange(w, dtype=np.float32) * sx + ox
        else:
            rng = np.array(cfg["anchor_ranges"][grp[0]], np.float32)
            zc = np.linspace(rng[2], rng[5], d, dtype=np.float32)
            yc = np.linspace(rng[1], rng[4], h, dtype=np.float32)
            xc = np.linspace(rng[0], rng[3], w, dtype=np.float32)
        nd = 7 + len(custom[gi])
        a = np.zeros((len(grp), len(rots), d, h, w, nd), np.float32)
        a[..., 7:] = custom[gi]
        a[..., 0] = xc[None, None, None, None, :]
        a[..., 1] = yc[None, None, None, :, None]
        a[..., 2] = zc[None, None, :, None, None]
        for si, sz in enumerate(grp):
            a[si, ..., 3:6] = np.array(cfg["anchor_sizes"][sz], np.float32)
        a[..., 6] = rots[None, :, None, None, None]
        out.append(a.reshape(-1, nd))
    return np.concatenate(out, 0)


# ------------------------------------------------------------------------------------------ modules
class SimpleVoxel(nn.Module):
    def __init__(self, num_input_features=4):
        super().__init__()
        self.num_input_features = num_input_features

    def forward(self, features, num_voxels, coors=None):
        s = features[:, :, :self.num_input_features].sum(dim=1)
        return (s / num_voxels.type_as(features).view(-1, 1)).contiguous()


class SimpleVoxelRadius(nn.Module):
    """voxel_encoder.py:228-255: the SimpleVoxel means with (x, y) replaced by their radius -- three channels, (r, z, w).
    ``forward`` is the module's own interface and ALWAYS returns those three columns (torch formulation: CPU tests, training, the
    module graph).  The device form is a method of its own, :meth:`rows4`: one launch (sec_simple_voxel_radius_f32) that writes rows
    of FOUR channels ``[r, z, w, 0]`` in ``out_dtype``; whoever uses it hands them to the sparse middle with ``in_pitch=4``, whose
    first conv then runs with its weight zero-padded 3 -> 4 input channels (SparseConvolution.pad_in_channels)."""

    ROW_PITCH = 4

    def __init__(self, num_input_features=4):
        super().__init__()
        self.num_input_features = num_input_features

    def forward(self, features, num_voxels, coors=None):
        nf = self.num_input_features
        mean = features[:, :, :nf].sum(dim=1) / num_voxels.type_as(features).view(-1, 1)
        radius = torch.linalg.vector_norm(mean[:, :2], ord=2, dim=1, keepdim=True)
        return torch.cat([radius, mean[:, 2:nf]], dim=1)

    def has_rows4(self, features):
        """the device kernel takes fp32 voxel tensors of >= 4 point features on the GPU, inference only"""
        return (features.is_cuda and features.dtype == torch.float32 and self.num_input_features == 4 and features.shape[2] >= 4
                and not torch.is_grad_enabled())

    def rows4(self, features, num_voxels, out_dtype=None, num_dev=None):
        return ops.simple_voxel_radius(features.contiguous(), num_voxels.int().contiguous(), self.num_input_features,
                                       out_dtype=out_dtype, num_dev=num_dev)

    def encode(self, features, num_voxels, out_dtype=None, num_dev=None):
        """-> (rows, in_pitch): the pitch-4 device rows where the kernel applies, else the three-column formulation (in_pitch None)."""
        if self.has_rows4(features):
            return self.rows4(features, num_voxels, out_dtype=out_dtype, num_dev=num_dev), self.ROW_PITCH
        rows = self.forward(features.float(), num_voxels)
        return (rows if out_dtype is None else rows.to(out_dtype)), None


class PFNLayer(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.linear = nn.Linear(cin, cout, bias=False)
        self.norm = nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01)


class PillarFeatureNet(nn.Module):
    """One-layer PillarFeatureNet (pointpillars.py:150-237); keys pfn_layers.0.{linear,norm}.  Inference on the
    GPU runs the fused sec_pfn_kind_fwd kernel, training on the GPU sec_pfn_kind_train_fwd / _bwd (ops.PFNTrainFunction: batch
    statistics, backward through the argmax; train_backend = "torch" selects the formulation below); the torch formulation serves
    CPU tests and as the autograd reference of the training kernels."""

    kind = ops.PFN_PLAIN        # the decorated row (ops.PFN_*; include/second_hip.h); the subclasses differ in nothing else

    def __init__(self, num_input_features=4, num_filters=(64,), voxel_size=(0.2, 0.2, 4), pc_range=(0, -40, -3, 70.4, 40, 1),
                 with_distance=False):
        super().__init__()
        assert len(num_filters) == 1, "the shipped PointPillars configs use a single PFN layer"
        self.with_distance = bool(with_distance)      # one more entry per row: the point's distance (see decorate)
        self._with_distance = self.with_distance      # (the reference's attribute name: what dropin.model_config reads)
        self.pfn_layers = nn.ModuleList([PFNLayer(num_input_features - 4 + ops.pfn_row_width(self.kind, self.with_distance),
                                                  num_filters[0])])
        self.vx, self.vy = voxel_size[0], voxel_size[1]
        self.x_offset, self.y_offset = self.vx / 2 + pc_range[0], self.vy / 2 + pc_range[1]

    train_backend = "hip"       # "torch": the reference's materialised [P, T, C] formulation in training (A/B, tests)

    def folded(self):
        """(W^T, scale, shift) of Linear + BatchNorm1d in eval mode; cached until one of the five tensors changes (in-place updates
        and load_state_dict bump their version counters): six element-wise launches per forward otherwise."""
        l = self.pfn_layers[0]
        src = (l.linear.weight, l.norm.weight, l.norm.bias, l.norm.running_mean, l.norm.running_var)
        key = tuple((t.data_ptr(), t._version) for t in src)
        cached = getattr(self, "_folded", None)
        if cached is None or cached[0] != key:
            with torch.no_grad():
                scale = (l.norm.weight * torch.rsqrt(l.norm.running_var + l.norm.eps)).float()
                shift = (l.norm.bias - l.norm.running_mean * scale).float()
                cached = self._folded = (key, (l.linear.weight.detach().t().contiguous().float(), scale.detach().contiguous(),
                                               shift.detach().contiguous()))
        return cached[1]

    def forward_slots(self, points, vox, out_dtype=None, num_dev=None):
        """Inference straight from the voxeliser's point lists (``vox`` = generate_device(points, ..., fill=False)): the
        [P, T, 4] pillar tensor is neither written nor read; bit-identical to :meth:`forward` on the materialised pillars."""
        wt, scale, shift = self.folded()
        return ops.pfn_forward_slots(points, vox, wt, scale, shift, self.vx, self.vy, self.x_offset, self.y_offset,
                                     out_dtype=out_dtype, num_dev=num_dev, kind=self.kind, with_distance=self.with_distance)

    def _forward_train_kernels(self, features, num_voxels, coors, num_dev=None):
        """Training on the device (sec_pfn_kind_train_fwd / _bwd on this class's row: batch statistics, argmax backward, no
        [P, T, C] tensor), or None where the torch formulation has to serve: CPU, eval / frozen or non-affine norm, a linear bias,
        train_backend = "torch", a shape the kernels do not take, no pillars.  ``num_dev``: static-capacity pillars with the count
        on the device; the torch formulation cannot serve those, so falling through is an error."""
        l = self.pfn_layers[0]
        bn = l.norm
        if not (features.is_cuda and self.training and bn.training and bn.track_running_stats and bn.affine and l.linear.bias is None
                and self.train_backend == "hip" and ops.pfn_train_supported(features, bn.num_features)
                and features.shape[0] > 0):
            if num_dev is not None:
                raise RuntimeError(f"{type(self).__name__}: a device-side pillar count (num_dev) in training mode needs the HIP "
                                   "training kernels (GPU, train_backend = 'hip', affine tracked BatchNorm, T <= 127, C <= 64)")
            return None
        mom = bn.momentum if bn.momentum is not None else 0.1
        fn = ops.pfn_kind_train_function(self.kind, self.with_distance)
        out = fn.apply(features.contiguous(), num_voxels, coors.int(), l.linear.weight, bn.weight, bn.bias, bn.running_mean,
                       bn.running_var, bn.eps, mom, (self.vx, self.vy, self.x_offset, self.y_offset),
                       *(() if num_dev is None else (num_dev,)))
        ops.bump_bn_counter(bn)
        return out

    def forward(self, features, num_voxels, coors, out_dtype=None, num_dev=None):
        if features.is_cuda and not self.training and not torch.is_grad_enabled():
            wt, scale, shift = self.folded()
            return ops.pfn_forward(features.float().contiguous(), num_voxels.int(), coors.int(), wt, scale, shift, self.vx,
                                   self.vy, self.x_offset, self.y_offset, out_dtype=out_dtype, num_dev=num_dev, kind=self.kind,
                                   with_distance=self.with_distance)
        out = self._forward_train_kernels(features, num_voxels, coors, num_dev)
        if out is not None:
            return out
        return self._forward_torch(features, num_voxels, coors)

    def decorate(self, features, num_voxels, coors):
        """The decorated, masked rows [P, T, K] of this class's kind in torch -- the formulation for the CPU, for autograd through eval
        mode and for train_backend = "torch"; the table of include/second_hip.h (SEC_PFN_*).  ``features`` is only read: the
        reference's PillarFeatureNetOld writes the centre offsets into the caller's x, y columns (a second call on the same example
        centres twice there); here the centred columns are new tensors."""
        n = num_voxels.to(features.dtype).view(-1, 1, 1)
        xyz = features[:, :, :3]
        mean = xyz.sum(1, keepdim=True) / n
        cx = coors[:, 3].to(features.dtype).view(-1, 1) * self.vx + self.x_offset
        cy = coors[:, 2].to(features.dtype).view(-1, 1) * self.vy + self.y_offset
        centre = torch.stack([features[:, :, 0] - cx, features[:, :, 1] - cy], -1)
        if self.kind in (ops.PFN_RADIUS, ops.PFN_RADIUS_HEIGHT):
            raw = torch.cat([torch.linalg.vector_norm(features[:, :, :2], ord=2, dim=2, keepdim=True), features[:, :, 2:]], -1)
        elif self.kind == ops.PFN_OLD:
            raw = torch.cat([centre, features[:, :, 2:]], -1)
        else:
            raw = features
        parts = [raw, xyz - mean, centre]
        if self.kind == ops.PFN_RADIUS_HEIGHT:        # max z - min z over ALL slots of the tensor, the padded zeros among them
            z = features[:, :, 2:3]
            parts.append((z.max(dim=1, keepdim=True)[0] - z.min(dim=1, keepdim=True)[0]).expand_as(z))
        if self.with_distance:                        # over the first three columns as the reference holds them: Old's are centred
            first3 = raw[:, :, :3] if self.kind == ops.PFN_OLD else xyz
            parts.append(torch.linalg.vector_norm(first3, ord=2, dim=2, keepdim=True))
        dec = torch.cat(parts, -1)
        t = features.shape[1]
        mask = (torch.arange(t, device=features.device).view(1, -1) < num_voxels.view(-1, 1)).to(features.dtype)
        return dec * mask.unsqueeze(-1)

    def _forward_torch(self, features, num_voxels, coors):
        l = self.pfn_layers[0]
        x = l.linear(self.decorate(features, num_voxels, coors))
        x = F.relu(l.norm(x.permute(0, 2, 1)).permute(0, 2, 1))
        return x.max(dim=1)[0]


class PillarFeatureNetRadius(PillarFeatureNet):
    """One-layer PillarFeatureNetRadius (pointpillars.py:240-325; nuscenes/all.pp.mhead): the raw (x, y) of every point give way to
    their radius, so the layer is Linear(num_input_features + 4, C); same keys pfn_layers.0.{linear,norm}.  sec_pfn_kind_* with
    SEC_PFN_RADIUS (in training ops.PFNRadiusTrainFunction), under the conditions of PillarFeatureNet."""
    kind = ops.PFN_RADIUS


class PillarFeatureNetOld(PillarFeatureNet):
    """One-layer PillarFeatureNetOld (pointpillars.py:68-151; nuscenes/all.pp.mida, all.pp.deprecated): the centre offsets stand in
    the raw x, y columns as well -- [x - cx, y - cy, z, w, x - mx, y - my, z - mz, x - cx, y - cy] -- because the reference writes
    them through a view of its input, after it took the cluster mean on the raw x, y.  Linear(num_input_features + 5, C), keys
    pfn_layers.0.{linear,norm}; sec_pfn_kind_fwd / _fwd_slots / _train_fwd / _train_bwd with SEC_PFN_OLD.  The reference's side
    effect is NOT reproduced: the caller's ``voxels`` are never written (there a second call on the same example centres twice)."""
    kind = ops.PFN_OLD


class PillarFeatureNetRadiusHeight(PillarFeatureNet):
    """One-layer PillarFeatureNetRadiusHeight (pointpillars.py:328-417): PillarFeatureNetRadius' row with the pillar's height h =
    max z - min z appended, taken over all T slots of the pillar tensor (the zero z of a padded slot takes part, as in the
    reference's min / max over dim 1) and masked to zero on padded slots like every entry.  Linear(num_input_features + 5, C);
    sec_pfn_kind_* with SEC_PFN_RADIUS_HEIGHT."""
    kind = ops.PFN_RADIUS_HEIGHT


class PointPillarsScatter(nn.Module):
    """pointpillars.py:420-476: pillars -> [B, C, ny, nx] pseudo image, one launch (sec_pillar_scatter)."""

    def __init__(self, output_shape, num_input_features=64):
        super().__init__()
        self.ny, self.nx, self.nchannels = int(output_shape[2]), int(output_shape[3]), num_input_features

    def forward(self, voxel_features, coords, batch_size, channels_last=False, num_dev=None):
        if torch.is_grad_enabled() and voxel_features.requires_grad:   # training: differentiable scatter
            from spconv.functional import PillarScatterFunction
            return PillarScatterFunction.apply(voxel_features.contiguous(), coords.int().contiguous(), batch_size,
                                               self.ny, self.nx, channels_last, *(() if num_dev is None else (num_dev,)))
        return ops.pillar_scatter(voxel_features.contiguous(), coords.int().contiguous(), batch_size, self.ny, self.nx,
                                  channels_last=channels_last, num_dev=num_dev)


def _bn1d(c):
    return nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)


def _bn2d(c):
    return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)


class SpMiddleFHD(nn.Module):
    """14 sparse conv layers; channel plan 4-16-16-32-32-32-64-...-64; state_dict keys
    ``middle_conv.<i>.weight`` as in the reference."""

    def __init__(self, output_shape, num_input_features=4):
        super().__init__()
        self.sparse_shape = [int(output_shape[1]) + 1, int(output_shape[2]), int(output_shape[3])]
        sub = lambda i, o, key: spconv.SubMConv3d(i, o, 3, bias=False, indice_key=key)
        down = lambda i, o, k, s, p: spconv.SparseConv3d(i, o, k, s, padding=p, bias=False)
        layers = []

        def add(conv, c):
            layers.extend([conv, _bn1d(c), nn.ReLU()])
        add(sub(num_input_features, 16, "subm0"), 16)
        add(sub(16, 16, "subm0"), 16)
        add(down(16, 32, 3, 2, 1), 32)
        add(sub(32, 32, "subm1"), 32)
        add(sub(32, 32, "subm1"), 32)
        add(down(32, 64, 3, 2, 1), 64)
        for _ in range(3):
            add(sub(64, 64, "subm2"), 64)
        add(down(64, 64, 3, 2, [0, 1, 1]), 64)
        for _ in range(3):
            add(sub(64, 64, "subm3"), 64)
        add(down(64, 64, (3, 1, 1), (2, 1, 1), 0), 64)
        self.middle_conv = spconv.SparseSequential(*layers)
        self.fused_chain = True       # static inference: all eight rulebooks from one fused build (SparseSequential.plan_chain)

    def forward(self, voxel_features, coors, batch_size, channels_last=False, num_active_dev=None, site_table=None, bev_sparse=False,
                in_pitch=None):
        """``in_pitch``: the caller declares that ``voxel_features`` are rows of that many channels padded with zeros behind the
        layer's input channels (SimpleVoxelRadius.rows4: 4); the first conv must have been built for it (pad_in_channels).
        ``site_table``: the ``site_table`` entry of the ops.voxelize result these (unfiltered) coors come from -- the first
        SubM rulebook then looks its sites up in the voxeliser's hash table instead of hashing them again.
        ``bev_sparse``: return a :class:`SparseBEV` (rows + indices) instead of the dense image when the output grid allows it."""
        x = spconv.SparseConvTensor(voxel_features, coors.int(), self.sparse_shape, batch_size,
                                    num_active_dev=num_active_dev)
        if in_pitch is not None:
            x.in_pitch = int(in_pitch)
        if site_table is not None and x.indices.data_ptr() == coors.data_ptr():
            x.site_table = ((x.indices.data_ptr(), x.indices.shape[0]), site_table)
        if num_active_dev is not None and self.fused_chain:
            x.planned = self.middle_conv.plan_chain(x)       # None: layer-by-layer builds
        x = self.middle_conv(x)
        self.last_overflow_checks = x.overflow_checks
        if channels_last and bev_sparse and x.features.shape[1] == 64 and int(x.spatial_shape[0]) == 2:
            return SparseBEV(x)                      # the RPN's first conv gathers from the rows: no dense image
        if channels_last:
            return x.dense_channels_last_2d()
        d = x.dense()
        n, c, dd, h, w = d.shape
        return d.view(n, c * dd, h, w)


# Layer plans of the reference's other sparse middles: ("subm", cout, indice_key) | ("down", cout, kernel, stride, padding).
MIDDLE_PLANS = {
    # middle.py:418-483: four strided convs, no SubM level; z 41 -> 21 -> 11 -> 5 -> 2, (y, x) / 8
    "SpMiddleFHDLite": [("down", 16, 3, 2, 1), ("down", 32, 3, 2, 1), ("down", 64, 3, 2, [0, 1, 1]), ("down", 64, (3, 1, 1), (2, 1, 1), 0)],
    # middle.py:213-300: SpMiddleFHD minus one stride-2 level; z 21 -> 11 -> 5 -> 2, (y, x) / 4
    "SpMiddleFHDPeople": [("subm", 16, "subm0"), ("subm", 16, "subm0"), ("down", 32, 3, 2, 1),
                          ("subm", 32, "subm1"), ("subm", 32, "subm1"), ("down", 64, 3, 2, [0, 1, 1]),
                          ("subm", 64, "subm2"), ("subm", 64, "subm2"), ("subm", 64, "subm2"), ("down", 64, (3, 1, 1), (2, 1, 1), 0)],
}


class SpMiddlePlanned(SpMiddleFHD):
    """A sparse middle built from a row of MIDDLE_PLANS: same state-dict keys (``middle_conv.<3 i>.weight``, BatchNorm1d at 3 i + 1),
    forward, fused rulebook chain and SparseBEV output as :class:`SpMiddleFHD`.  A first layer with fewer than four input channels
    (SimpleVoxelRadius' three) keeps the reference's weight shape and takes the encoder's pitch-4 rows (pad_in_channels)."""

    plan_name = None

    def __init__(self, output_shape, num_input_features=4):
        nn.Module.__init__(self)
        self.sparse_shape = [int(output_shape[1]) + 1, int(output_shape[2]), int(output_shape[3])]
        layers, cin = [], int(num_input_features)
        for spec in MIDDLE_PLANS[self.plan_name]:
            if spec[0] == "subm":
                conv = spconv.SubMConv3d(cin, spec[1], 3, bias=False, indice_key=spec[2])
            else:
                conv = spconv.SparseConv3d(cin, spec[1], spec[2], spec[3], padding=spec[4], bias=False)
            cin = spec[1]
            layers.extend([conv, _bn1d(cin), nn.ReLU()])
        if num_input_features < 4:
            layers[0].pad_in_channels = 4
        self.middle_conv = spconv.SparseSequential(*layers)
        self.fused_chain = True


class SpMiddleFHDLite(SpMiddlePlanned):
    plan_name = "SpMiddleFHDLite"


class SpMiddleFHDPeople(SpMiddlePlanned):
    plan_name = "SpMiddleFHDPeople"


VFES = {"SimpleVoxel": SimpleVoxel, "SimpleVoxelRadius": SimpleVoxelRadius, "PillarFeatureNet": PillarFeatureNet,
        "PillarFeatureNetRadius": PillarFeatureNetRadius, "PillarFeatureNetOld": PillarFeatureNetOld,
        "PillarFeatureNetRadiusHeight": PillarFeatureNetRadiusHeight}
PILLAR_VFES = ("PillarFeatureNet", "PillarFeatureNetRadius", "PillarFeatureNetOld", "PillarFeatureNetRadiusHeight")
MIDDLES = {"SpMiddleFHD": SpMiddleFHD, "SpMiddleFHDLite": SpMiddleFHDLite, "SpMiddleFHDPeople": SpMiddleFHDPeople}


class SparseBEV:
    """The sparse middle's output handed to RPNInference WITHOUT ``.dense()``: rows + (b, z, y, x) indices of a [2, H, W] grid.
    ``dense()`` gives the reference's [B, C * D, H, W] channels_last tensor (middle.py:206-210) for consumers that need it."""

    def __init__(self, sp):
        self.sp = sp
        self.features, self.indices, self.num_dev = sp.features, sp.indices, sp.num_active_dev
        self.batch_size, self.spatial_shape = sp.batch_size, [int(v) for v in sp.spatial_shape]

    def site_map(self):
        m = getattr(self.sp, "site_map_tensor", None)
        if m is not None:                            # written by the fused rulebook chain's tables launch
            return m
        # rows numbered by the sorted build of the last strided layer: the map is that build's bitmap ranks (one launch)
        tbl = getattr(self.sp, "site_bitmap", None)
        if (tbl is not None and tbl[0] == (self.indices.data_ptr(), self.indices.shape[0]) and isinstance(tbl[1][0], str)
                and tbl[1][0] == "sorted"):
            tbl[1][1].record_stream(torch.cuda.current_stream())
            return ops.sparse_site_map_sorted(tbl[1][1], self.indices.shape[0], self.batch_size, self.spatial_shape, num_dev=self.num_dev)
        return ops.sparse_site_map(self.indices, self.batch_size, self.spatial_shape, num_dev=self.num_dev)

    def tile_lists(self, layers, masks=False, cover=False):
        """(order, counts[, nbr_masks | TileCover]) of ops.rpn_tile_live for the first ``layers`` RPN convs, computed once per tensor: whoever asks
        first decides where the launch sits (the sparse segment of a staged capture, so that it stays out of the serialised RPN segment)."""
        t = getattr(self, "_tile_lists", None)
        key = (layers, bool(masks), bool(cover))
        if t is None or t[0] != key:
            t = self._tile_lists = (key, ops.rpn_tile_live(self.site_map(), layers, masks=bool(masks), cover=bool(cover)))
        return t[1]

    def dense(self):
        return self.sp.dense_channels_last_2d()


class PillarBEV:
    """The PillarFeatureNet's rows handed to RPNInference WITHOUT PointPillarsScatter's canvas (pointpillars.py:444-476): rows + (b, z, y, x)
    coordinates of an [ny, nx] grid.  ``dense()`` is the scatter's channels_last image for consumers that need it."""

    def __init__(self, features, coords, batch_size, ny, nx, num_dev=None):
        self.features, self.coords, self.num_dev = features.contiguous(), coords.int().contiguous(), num_dev
        self.batch_size, self.ny, self.nx = int(batch_size), int(ny), int(nx)

    def site_map(self):
        return ops.pillar_site_map(self.coords, self.batch_size, self.ny, self.nx, num_dev=self.num_dev)

    def dense(self):
        return ops.pillar_scatter(self.features, self.coords, self.batch_size, self.ny, self.nx, channels_last=True, num_dev=self.num_dev)


class RPNV2(nn.Module):
    """ZeroPad+Conv3x3+BN+ReLU, layer_num x (Conv3x3+BN+ReLU) per block; deconv (or strided conv) per
    block; three 1x1 heads.  Keys: blocks.<b>.<i>, deblocks.<b>.<i>, conv_cls, conv_box, conv_dir_cls."""

    def __init__(self, num_class=1, layer_nums=(5,), layer_strides=(1,), num_filters=(128,), upsample_strides=(1,),
                 num_upsample_filters=(128,), num_input_features=128, num_anchor_per_loc=2, box_code_size=7,
                 num_direction_bins=2, use_direction_classifier=True):
        super().__init__()
        self._num_anchor_per_loc, self._num_class = num_anchor_per_loc, num_class
        self._box_code_size, self._num_direction_bins = box_code_size, num_direction_bins
        self._use_direction_classifier = use_direction_classifier
        self._upsample_start_idx = len(layer_nums) - len(upsample_strides)
        blocks, deblocks = [], []
        cin = num_input_features
        for i, n in enumerate(layer_nums):
            planes = num_filters[i]
            mods = [nn.ZeroPad2d(1), nn.Conv2d(cin, planes, 3, stride=layer_strides[i], bias=False), _bn2d(planes), nn.ReLU()]
            for _ in range(n):
                mods += [nn.Conv2d(planes, planes, 3, padding=1, bias=False), _bn2d(planes), nn.ReLU()]
            blocks.append(nn.Sequential(*mods))
            if i - self._upsample_start_idx >= 0:
                s = upsample_strides[i - self._upsample_start_idx]
                cup = num_upsample_filters[i - self._upsample_start_idx]
                if s >= 1:
                    s = int(round(s))
                    up = nn.ConvTranspose2d(planes, cup, s, stride=s, bias=False)
                else:
                    s = int(round(1 / s))
                    up = nn.Conv2d(planes, cup, s, stride=s, bias=False)
                deblocks.append(nn.Sequential(up, _bn2d(cup), nn.ReLU()))
            cin = planes
        self.blocks, self.deblocks = nn.ModuleList(blocks), nn.ModuleList(deblocks)
        final = sum(num_upsample_filters) if len(num_upsample_filters) else cin
        self.conv_cls = nn.Conv2d(final, num_anchor_per_loc * num_class, 1)
        self.conv_box = nn.Conv2d(final, num_anchor_per_loc * box_code_size, 1)
        if use_direction_classifier:
            self.conv_dir_cls = nn.Conv2d(final, num_anchor_per_loc * num_direction_bins, 1)

    def forward(self, x):
        ups = []
        for i, blk in enumerate(self.blocks):
            x = blk(x)
            if i - self._upsample_start_idx >= 0:
                ups.append(self.deblocks[i - self._upsample_start_idx](x))
        if ups:
            x = torch.cat(ups, dim=1) if len(ups) > 1 else ups[0]
        a = self._num_anchor_per_loc

        def head(conv, code):
            y = conv(x)
            h, w = y.shape[2:]
            return y.view(-1, a, code, h, w).permute(0, 1, 3, 4, 2).contiguous()
        ret = {"box_preds": head(self.conv_box, self._box_code_size), "cls_preds": head(self.conv_cls, self._num_class)}
        if self._use_direction_classifier:
            ret["dir_cls_preds"] = head(self.conv_dir_cls, self._num_direction_bins)
        return ret


class RPNNoHead(nn.Module):
    """The trunk of RPNV2 without heads (rpn.py:202-331, 500-529): same blocks / deblocks and keys; forward returns every block's
    output ("stage<i>"), every deblock's ("up<i>") and their concatenation ("out").  The heads belong to the network
    (net_multi_head.py: SmallObjectHead on stage0, DefaultHead on out)."""

    def __init__(self, num_class=2, layer_nums=(3, 5, 5), layer_strides=(2, 2, 2), num_filters=(128, 128, 256), upsample_strides=(1, 2, 4),
                 num_upsample_filters=(256, 256, 256), num_input_features=128, num_anchor_per_loc=2, box_code_size=7,
                 num_direction_bins=2, use_direction_classifier=True):
        super().__init__()
        self._layer_nums, self._layer_strides, self._num_filters = list(layer_nums), list(layer_strides), list(num_filters)
        self._upsample_strides, self._num_upsample_filters = list(upsample_strides), list(num_upsample_filters)
        self._num_input_features, self._use_norm, self._use_groupnorm = num_input_features, True, False
        self._use_direction_classifier = use_direction_classifier
        trunk = RPNV2(num_class, layer_nums, layer_strides, num_filters, upsample_strides, num_upsample_filters, num_input_features,
                      num_anchor_per_loc, box_code_size, num_direction_bins, use_direction_classifier)
        self.blocks, self.deblocks, self._upsample_start_idx = trunk.blocks, trunk.deblocks, trunk._upsample_start_idx

    def forward(self, x):
        ups, res = [], {}
        for i, blk in enumerate(self.blocks):
            x = blk(x)
            res[f"stage{i}"] = x
            if i - self._upsample_start_idx >= 0:
                ups.append(self.deblocks[i - self._upsample_start_idx](x))
        for i, up in enumerate(ups):
            res[f"up{i}"] = up
        res["out"] = torch.cat(ups, dim=1) if ups else x
        return res


class DefaultHead(nn.Module):
    """net_multi_head.py:74-119: the three 1x1 heads on a feature map; predictions flattened to [B, A * H * W, code]."""

    def __init__(self, num_filters, num_class, num_anchor_per_loc, box_code_size=7, num_direction_bins=2, use_direction_classifier=True,
                 encode_background_as_zeros=True):
        super().__init__()
        assert encode_background_as_zeros, "sigmoid scores without a background class (every shipped config)"
        self._num_anchor_per_loc, self._num_class, self._box_code_size = num_anchor_per_loc, num_class, box_code_size
        self._num_direction_bins, self._use_direction_classifier = num_direction_bins, use_direction_classifier
        self._build_heads(int(num_filters))

    def _build_heads(self, cin):
        a = self._num_anchor_per_loc
        self.conv_cls = nn.Conv2d(cin, a * self._num_class, 1)
        self.conv_box = nn.Conv2d(cin, a * self._box_code_size, 1)
        if self._use_direction_classifier:
            self.conv_dir_cls = nn.Conv2d(cin, a * self._num_direction_bins, 1)

    def features(self, x):
        return x

    def forward(self, x):
        x = self.features(x)
        b, a = x.shape[0], self._num_anchor_per_loc

        def head(conv, code):
            y = conv(x)
            h, w = y.shape[2:]
            return y.view(-1, a, code, h, w).permute(0, 1, 3, 4, 2).contiguous().view(b, -1, code)
        ret = {"box_preds": head(self.conv_box, self._box_code_size), "cls_preds": head(self.conv_cls, self._num_class)}
        if self._use_direction_classifier:
            ret["dir_cls_preds"] = head(self.conv_dir_cls, self._num_direction_bins)
        return ret


class SmallObjectHead(DefaultHead):
    """net_multi_head.py:14-71: three Conv2d(3x3, pad 1) + BatchNorm2d + ReLU of 64 channels (``net``), then the 1x1 heads.  The
    norms are torch's DEFAULT nn.BatchNorm2d(64) -- eps 1e-5, momentum 0.1 -- not the eps 1e-3 of every other norm of the network."""

    def __init__(self, num_filters, num_class, num_anchor_per_loc, box_code_size=7, num_direction_bins=2, use_direction_classifier=True,
                 encode_background_as_zeros=True):
        nn.Module.__init__(self)
        assert encode_background_as_zeros, "sigmoid scores without a background class (every shipped config)"
        self._num_anchor_per_loc, self._num_class, self._box_code_size = num_anchor_per_loc, num_class, box_code_size
        self._num_direction_bins, self._use_direction_classifier = num_direction_bins, use_direction_classifier
        mods, cin = [], int(num_filters)
        for _ in range(3):
            mods += [nn.Conv2d(cin, 64, 3, bias=False, padding=1), nn.BatchNorm2d(64), nn.ReLU()]
            cin = 64
        self.net = nn.Sequential(*mods)
        self._build_heads(64)

    def features(self, x):
        return self.net(x)


def stage0_crop(height):
    """Cells the multi-head network cuts from every side of block 0's output before the small-object head: round(0.1 * H) with
    numpy's rounding, taken from the HEIGHT and applied to both axes (net_multi_head.py:163-165).  0 would make the reference slice
    ``[0:-0]`` -- an empty tensor: refused."""
    c = int(np.round(height * 0.1))
    if c == 0:
        raise ValueError(f"multi-head network: stage0 crop round(0.1 * {height}) is 0 (the reference's slice [0:-0] is empty); "
                         "block 0's output must be at least 5 cells high")
    return c


RPN_TRAIN_BACKEND = "hip"


def _mixed_block(blk, x, dtype, use_hip):
    """One block of Conv2d / BatchNorm2d / ReLU modules for :func:`rpn_forward_mixed`: 128-channel stride-1 3x3 triples on the
    hand-written kernels, everything else on torch under autocast."""
    mods = list(blk.children())
    i, pad = 0, 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.ZeroPad2d):
            pad = m.padding[0]
            i += 1
            continue
        fused = (use_hip and isinstance(m, nn.Conv2d) and i + 2 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d)
                 and isinstance(mods[i + 2], nn.ReLU) and m.bias is None and m.kernel_size == (3, 3) and m.stride == (1, 1)
                 and m.padding[0] + pad == 1 and m.padding[1] + pad == 1 and m.dilation == (1, 1) and m.groups == 1
                 and ops.conv2d_wgrad_supported(m.in_channels, m.out_channels, 3, 1, 1, dtype) and mods[i + 1].training
                 and mods[i + 1].track_running_stats and mods[i + 1].affine)
        if fused:
            bn = mods[i + 1]
            y = ops.Conv3x3Function.apply(x, m.weight)
            mom = bn.momentum if bn.momentum is not None else 0.1
            x = ops.BatchNormReluFunction.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, mom, True)
            ops.bump_bn_counter(bn)
            i, pad = i + 3, 0
            continue
        with torch.autocast("cuda", dtype=dtype, enabled=x.is_cuda, cache_enabled=False):
            if pad:
                x = F.pad(x, (pad, pad, pad, pad))
                pad = 0
            x = m(x)
        i += 1
    return x


def _mixed_deblock(deb, x, dtype, use_hip):
    """One deblock the same way: the 128 -> 128 1x1 transposed convolution on the hand-written kernels, others on torch."""
    mods = list(deb.children())
    m = mods[0]
    if (use_hip and len(mods) == 3 and isinstance(m, nn.ConvTranspose2d) and isinstance(mods[1], nn.BatchNorm2d)
            and isinstance(mods[2], nn.ReLU) and m.bias is None and m.kernel_size == (1, 1) and m.stride == (1, 1)
            and m.padding == (0, 0) and m.output_padding == (0, 0) and m.groups == 1 and m.in_channels == 128
            and m.out_channels == 128 and dtype in (torch.bfloat16, torch.float16) and mods[1].training
            and mods[1].track_running_stats and mods[1].affine):
        bn = mods[1]
        y = ops.ConvTranspose1x1Function.apply(x, m.weight)
        mom = bn.momentum if bn.momentum is not None else 0.1
        z = ops.BatchNormReluFunction.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, mom, True)
        ops.bump_bn_counter(bn)
        return z
    with torch.autocast("cuda", dtype=dtype, enabled=x.is_cuda, cache_enabled=False):
        return deb(x)


def _mixed_trunk(rpn, x, dtype, use_hip):
    """The walk over ``rpn.blocks`` / ``rpn.deblocks`` shared by :func:`rpn_forward_mixed` and :func:`multihead_forward_mixed`:
    (every block's output, every deblock's output)."""
    stages, ups = [], []
    for i, blk in enumerate(rpn.blocks):
        x = _mixed_block(blk, x, dtype, use_hip)
        stages.append(x)
        if i - rpn._upsample_start_idx >= 0:
            ups.append(_mixed_deblock(rpn.deblocks[i - rpn._upsample_start_idx], x, dtype, use_hip))
    return stages, ups


def rpn_forward_mixed(rpn, x, dtype, loss_args=None, loss_terms=False):
    """Training forward of an RPNV2 with 16-bit activations over its fp32 master weights (the DeviceTrainer's amp path).  Every
    Conv2d(128, 128, 3, stride 1) + BatchNorm2d + ReLU triple of the blocks runs on the hand-written kernels -- forward and data
    gradient on k_conv2d_halo_reg, weight gradient on k_conv2d_wgrad3x3, BatchNorm (batch statistics) + ReLU fused
    (ops.Conv3x3Function / ops.BatchNormReluFunction; rpn.py:486-497 trained by train.py:316-322); anything else (strided or
    other-width convs, the deblocks, the 1x1 heads) stays on torch under autocast.  ``models.RPN_TRAIN_BACKEND = "miopen"``: all of it
    on torch (the round-2 path; tests compare the two).  Same arithmetic as RPNV2.forward up to 16-bit rounding of the activations.  (autocast's
    weight-cast cache is off: the function is captured into hipGraphs by DeviceTrainer, and a cached cast made during capture
    would be stale on replay.)
    ``loss_args`` = (labels, reg_targets, anchors, importance, loss_cfg): when the heads run as one stacked convolution and the loss
    kernel has that head shape, the loss is taken from the stacked tensor (ops.HeadsLossFunction) and {"loss", "out6"} comes back
    instead of the three prediction tensors; ``loss_terms``: plus "cls_preds" / "cls_loss" / "loc_loss", the per-anchor fp32 tensors of the
    reference's loss dict (voxelnet.py:299-309), from the same launch."""
    use_hip = RPN_TRAIN_BACKEND == "hip" and x.is_cuda
    x = x.to(dtype).contiguous(memory_format=torch.channels_last)
    stages, ups = _mixed_trunk(rpn, x, dtype, use_hip)
    x = stages[-1]
    heads = [(rpn.conv_box, rpn._box_code_size, "box_preds"), (rpn.conv_cls, rpn._num_class, "cls_preds")]
    if rpn._use_direction_classifier:
        heads.append((rpn.conv_dir_cls, rpn._num_direction_bins, "dir_cls_preds"))
    a = rpn._num_anchor_per_loc
    if (use_hip and len(ups) == 1 and ups[0].shape[1] == 128 and dtype in (torch.bfloat16, torch.float16)
            and sum(c.out_channels for c, _, _ in heads) <= 64
            and all(isinstance(c, nn.Conv2d) and c.kernel_size == (1, 1) and c.stride == (1, 1) and c.padding == (0, 0) and c.bias is not None
                    and c.in_channels == 128 for c, _, _ in heads)):
        # the three heads as one 128 -> 64 1x1 convolution (output channels stacked, zero padded) on the hand-written kernels
        tot = sum(c.out_channels for c, _, _ in heads)
        wd = heads[0][0].weight
        pads = getattr(rpn, "_sec_head_pads", None)          # the zero rows of the stacked weight / bias: made once, not filled every step
        if pads is None or pads[0].shape[0] != 64 - tot or pads[0].device != wd.device or pads[0].dtype != wd.dtype:
            pads = (torch.zeros((64 - tot, 128, 1, 1), dtype=wd.dtype, device=wd.device), torch.zeros((64 - tot,), dtype=wd.dtype, device=wd.device))
            rpn._sec_head_pads = pads
        wcat = torch.cat([c.weight for c, _, _ in heads] + [pads[0]], 0)
        bcat = torch.cat([c.bias for c, _, _ in heads] + [pads[1]], 0)
        bins = rpn._num_direction_bins if rpn._use_direction_classifier else 0
        if (loss_args is not None and rpn._box_code_size == 7
                and ops.heads_loss_supported(64, a, rpn._num_class, bins, dtype)):
            # the loss straight from the stacked head tensor, its gradient straight back into it (ops.HeadsLossFunction)
            labels, reg_targets, anchors, importance, loss_cfg = loss_args
            res = ops.HeadsLossFunction.apply(ups[0].contiguous(memory_format=torch.channels_last), wcat, bcat, labels, reg_targets,
                                              anchors, importance, a, rpn._num_class, bins, loss_cfg, bool(loss_terms))
            out = {"loss": res[0], "out6": res[1]}
            if loss_terms:
                out.update(cls_preds=res[2], cls_loss=res[3], loc_loss=res[4])
            return out
        y = ops.Heads1x1Function.apply(ups[0].contiguous(memory_format=torch.channels_last), wcat, bcat)
        ret, c0 = {}, 0
        h, w = y.shape[2:]
        for conv, code, name in heads:
            o = y[:, c0:c0 + conv.out_channels]
            c0 += conv.out_channels
            ret[name] = o.reshape(-1, a, code, h, w).permute(0, 1, 3, 4, 2).contiguous()
        return ret
    with torch.autocast("cuda", dtype=dtype, enabled=x.is_cuda, cache_enabled=False):
        if ups:
            x = torch.cat(ups, dim=1) if len(ups) > 1 else ups[0]

        def head(conv, code):
            y = conv(x)
            h, w = y.shape[2:]
            return y.view(-1, a, code, h, w).permute(0, 1, 3, 4, 2).contiguous()
        ret = {"box_preds": head(rpn.conv_box, rpn._box_code_size), "cls_preds": head(rpn.conv_cls, rpn._num_class)}
        if rpn._use_direction_classifier:
            ret["dir_cls_preds"] = head(rpn.conv_dir_cls, rpn._num_direction_bins)
    return ret


def multihead_forward_mixed(det, x, dtype):
    """Training forward of a multi-head network's dense part (RPNNoHead trunk + large_head on "out" + small_head on the cropped
    "stage0"; net_multi_head.py:121-176) with ``dtype`` activations over the fp32 master weights: the multi-head sibling of
    :func:`rpn_forward_mixed`, on the same block walk.  The 128-channel stride-1 3x3 convolutions of the trunk take the hand-written
    forward / dgrad / wgrad kernels; block 0 and the small head's tower (64-channel 3x3 convolutions, which
    ops.conv2d_wgrad_supported does not cover; the tower's norms keep torch's eps 1e-5 / momentum 0.1), the strided convolutions,
    the deblocks and the 1x1 heads run on torch under autocast.  Returns box_preds / cls_preds / dir_cls_preds concatenated large
    head first, then small, flattened as DefaultHead.forward flattens them.  ``dtype`` = torch.float32 is the module graph's
    arithmetic (CPU tests)."""
    rpn = det.rpn
    use_hip = RPN_TRAIN_BACKEND == "hip" and x.is_cuda
    x = x.to(dtype)
    if x.is_cuda:       # the kernels' layout; off the GPU the input keeps its own, so that float32 there IS the module graph's arithmetic
        x = x.contiguous(memory_format=torch.channels_last)
    stages, ups = _mixed_trunk(rpn, x, dtype, use_hip)
    c = stage0_crop(stages[0].shape[2])
    small_in = stages[0][:, :, c:-c, c:-c]          # a plain slice: autograd pads the gradient
    tower = _mixed_block(det.small_head.net, small_in, dtype, use_hip)
    with torch.autocast("cuda", dtype=dtype, enabled=x.is_cuda, cache_enabled=False):
        out = torch.cat(ups, dim=1) if len(ups) > 1 else ups[0]
        parts = []
        for head, feat in ((det.large_head, out), (det.small_head, tower)):
            b, a = feat.shape[0], head._num_anchor_per_loc

            def flat(conv, code):
                y = conv(feat)
                h, w = y.shape[2:]
                return y.view(-1, a, code, h, w).permute(0, 1, 3, 4, 2).contiguous().view(b, -1, code)
            p = {"box_preds": flat(head.conv_box, head._box_code_size), "cls_preds": flat(head.conv_cls, head._num_class)}
            if head._use_direction_classifier:
                p["dir_cls_preds"] = flat(head.conv_dir_cls, head._num_direction_bins)
            parts.append(p)
    return {k: torch.cat([p[k] for p in parts], dim=1) for k in parts[0]}


def fold_conv_bn_(seq):
    """In place: fold every (Conv2d|ConvTranspose2d, BatchNorm2d) pair of an nn.Sequential (eval mode)."""
    mods = list(seq.children())
    out = []
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d):
            bn = mods[i + 1]
            scale = bn.weight.float() * torch.rsqrt(bn.running_var.float() + bn.eps)
            shift = bn.bias.float() - bn.running_mean.float() * scale
            w = m.weight.float()
            if isinstance(m, nn.ConvTranspose2d):
                w = w * scale.view(1, -1, 1, 1)
            else:
                w = w * scale.view(-1, 1, 1, 1)
            b = shift if m.bias is None else m.bias.float() * scale + shift
            m.weight = nn.Parameter(w.to(m.weight.dtype), requires_grad=False)
            m.bias = nn.Parameter(b.to(m.weight.dtype), requires_grad=False)
            out.append(m)
            i += 2
        else:
            out.append(m)
            i += 1
    return nn.Sequential(*out)


EXACT_RPN_BACKENDS = ("torch", "hip")


def exact_rpn_default():
    """Process default of ``prepare_inference(exact=True, exact_rpn=None)``: the environment variable SEC_FP32_RPN, "torch" (the
    default: torch's fp32 convolutions) or "hip" (the fp32-MFMA kernels).  Any other value is an error, raised here."""
    v = os.environ.get("SEC_FP32_RPN", "torch")
    if v not in EXACT_RPN_BACKENDS:
        raise ValueError(f"SEC_FP32_RPN={v!r}: allowed values are 'torch' and 'hip'")
    return v


class _Fp32Arithmetic:
    """How RPNInference's fp32 block represents an activation map ``a`` ([B, 128, H, W] channels_last) and which ops compute on it: a
    (hi, lo) pair of bf16 planes, or one fp32 map.  Backgrounds and empty-frame maps are in the same representation."""

    def __init__(self, name, planes, pack, conv, conv_tiles, chain):
        self.name, self._planes, self._pack, self._conv, self._conv_tiles, self._chain = name, planes, pack, conv, conv_tiles, chain

    def _args(self, a):
        return a if self._planes == 2 else (a,)

    def pack(self, weight):
        """Folded fp32 weight [Cout, 128, k, k] -> the packed image the convs / the chain read; None for a shape they do not take."""
        return self._pack(weight)

    def zeros(self, h, w, device):
        """The input of a frame without sites."""
        z = torch.zeros((1, 128, h, w), dtype=torch.bfloat16 if self._planes == 2 else torch.float32, device=device)
        z = z.contiguous(memory_format=torch.channels_last)
        return (z, z.clone()) if self._planes == 2 else z

    def enter(self, x):
        return ops.split_bf16x2(x) if self._planes == 2 else x

    def leave(self, a):
        return ops.merge_bf16x2(*a) if self._planes == 2 else a

    def conv(self, a, packed, bias, cout, sparse_input=False):
        return self._conv(*self._args(a), packed, bias, cout, relu=True, sparse_input=sparse_input)

    def conv_tiles(self, a, packed, bias, cout, tile_order, live_counts, background, nbr_masks, background_in):
        return self._conv_tiles(*self._args(a), packed, bias, cout, tile_order, live_counts, background=background, relu=True,
                                nbr_masks=nbr_masks, background_in=background_in)

    def chain(self, a, w1, b1, w2, b2):
        """Deblock + merged heads (padded to 64 channels) in one launch: fp32 [B, 64, H, W] channels_last."""
        return self._chain(*self._args(a), w1, b1, w2, b2, 64, relu1=True)


# fp32 storage on the bf16 matrix pipe with split operands (v = hi + lo, three passes, fp32 accumulation): the fp32 default
_BF16X3 = _Fp32Arithmetic("bf16x3", 2, ops.conv2d_pack_weight_x3, ops.conv2d_nhwc_x3, ops.conv2d_nhwc_x3_tiles, ops.conv1x1_chain_x3)
# IEEE fp32 products on the fp32 MFMA (v_mfma_f32_32x32x2_f32): the exact mode's RPN
_FP32 = _Fp32Arithmetic("fp32", 1, ops.conv2d_pack_weight_f32, ops.conv2d_nhwc_f32, ops.conv2d_nhwc_f32_tiles, ops.conv1x1_chain_f32)


class RPNInference(nn.Module):
    """Inference form of a single-block RPNV2: BatchNorm2d folded into the conv weights (scale) and a float32
    bias, ZeroPad2d merged into the conv padding, the stride-1 1x1 ConvTranspose2d rewritten as a 1x1 conv, the three
    1x1 heads merged into one conv (output channels padded to a multiple of 64).  Every 3x3 conv runs on the
    hand-written MFMA kernel with bias + ReLU fused (sec_conv2d_nhwc), the deblock + heads as one fused kernel
    (sec_conv1x1_chain_nhwc); backend="miopen" keeps torch convs + one fused bias/ReLU pass for A/B runs.
    Same arithmetic as RPNV2.forward (rpn.py:314-331,393-420) up to bf16 rounding of the folded weights.
    A float32 network runs the same block in one of two fp32 arithmetics (``self.fp32``, a :class:`_Fp32Arithmetic`, with its packed
    weights in ``fp32_packed`` / ``fp32_chain``; None for the 16-bit and torch forms): "bf16x3" = split bf16 operands (backend="hip"),
    "fp32" = IEEE fp32 products on the fp32 MFMA (backend="hip_f32").  One forward, :meth:`_forward_fp32`, serves both."""

    @staticmethod
    def supports(rpn):
        """Every deblock must be expressible as a plain conv: Conv2d(k = s, stride = s) ("upsample" stride < 1), the
        stride-1 1x1 ConvTranspose2d, or ConvTranspose2d(k = s, stride = s), which is a 1x1 conv to s*s*Cout channels
        followed by a depth-to-space rearrangement."""
        for d in rpn.deblocks:
            m = list(d.children())[0]
            if isinstance(m, nn.ConvTranspose2d) and (m.kernel_size != m.stride or m.kernel_size[0] != m.kernel_size[1]
                                                      or m.padding != (0, 0) or m.output_padding != (0, 0)):
                return False
        # (a head-only tower -- _TowerAsRPN: one block, heads straight on its output -- has no deblock)
        return len(rpn.blocks) >= 1 and (len(rpn.deblocks) >= 1 or getattr(rpn, "_heads_on_last_block", False))

    def __init__(self, rpn, dtype, backend="hip", gather_first=True):
        """``backend``: "hip" = the hand-written MFMA convs (default), "miopen" = torch convolutions + one fused bias / ReLU pass (the
        phase-1 path: A/B yardstick).  ``gather_first``: the first conv reads the sparse rows through a site map instead of a dense
        image when the shapes allow (False: always the dense image)."""
        super().__init__()
        assert self.supports(rpn)
        self.a, self.codes = rpn._num_anchor_per_loc, (rpn._box_code_size, rpn._num_class, rpn._num_direction_bins)

        def fold(mods):
            out, pad, i = [], 0, 0
            while i < len(mods):
                m = mods[i]
                if isinstance(m, nn.ZeroPad2d):
                    pad = m.padding[0]
                elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                    bn = mods[i + 1]
                    assert isinstance(bn, nn.BatchNorm2d) and m.bias is None
                    scale = bn.weight.float() * torch.rsqrt(bn.running_var.float() + bn.eps)
                    bias = bn.bias.float() - bn.running_mean.float() * scale
                    w = m.weight.detach().float()
                    up = 1
                    if isinstance(m, nn.ConvTranspose2d):
                        # [Cin, Cout, s, s] -> 1x1 conv with output channel (dy*s + dx)*Cout + co; depth-to-space afterwards
                        up = m.kernel_size[0]
                        w = (w * scale.view(1, -1, 1, 1)).permute(2, 3, 1, 0).reshape(up * up * w.shape[1], w.shape[0], 1, 1)
                        bias = bias.repeat(up * up)
                        stride, padding = [1, 1], [0, 0]
                    else:
                        stride, padding = list(m.stride), [m.padding[0] + pad, m.padding[1] + pad]
                        w = w * scale.view(-1, 1, 1, 1)
                    w = w.to(dtype).contiguous(memory_format=torch.channels_last)
                    out.append((w, bias.detach().contiguous(), stride, padding, up))
                    pad = 0
                    i += 1
                i += 1
            return out
        # execution plan over a flat layer list: ("c", i) = conv layer i of a block, ("u", i) = deblock conv i whose output
        # is one of the concatenated feature maps
        layers, self.plan = [], []
        self.block_last = []             # layer index of every block's last conv
        self.stage0_layer = None         # a layer index: forward() also returns that conv's output as preds["stage0"] (MultiHeadInference)
        up0 = rpn._upsample_start_idx
        for bi, blk in enumerate(rpn.blocks):
            for l in fold(list(blk.children())):
                self.plan.append(("c", len(layers)))
                layers.append(l)
            self.block_last.append(len(layers) - 1)
            if bi - up0 >= 0:
                (l,) = fold(list(rpn.deblocks[bi - up0].children()))
                self.plan.append(("u", len(layers)))
                layers.append(l)
        single = len(rpn.blocks) == 1
        self.ws = nn.ParameterList([nn.Parameter(w, requires_grad=False) for w, _, _, _, _ in layers])
        self.bs = nn.ParameterList([nn.Parameter(b, requires_grad=False) for _, b, _, _, _ in layers])
        self.cfgs = [(s, p) for _, _, s, p, _ in layers]
        self.ups = [u for _, _, _, _, u in layers]      # depth-to-space factor after the conv (transposed deblocks)
        heads = [rpn.conv_box, rpn.conv_cls] + ([rpn.conv_dir_cls] if rpn._use_direction_classifier else [])
        self.splits = [h.out_channels for h in heads]
        tot = sum(self.splits)
        padc = (-tot) % 8
        hw = torch.cat([h.weight.detach().float() for h in heads] + [torch.zeros(padc, heads[0].in_channels, 1, 1, device=heads[0].weight.device)], 0)
        hb = torch.cat([h.bias.detach().float() for h in heads] + [torch.zeros(padc, device=heads[0].weight.device)], 0)
        self.head_w = nn.Parameter(hw.to(dtype).contiguous(memory_format=torch.channels_last), requires_grad=False)
        self.head_b = nn.Parameter(hb.contiguous(), requires_grad=False)
        convs = [i for kind, i in self.plan if kind == "c"]      # the block convs' layer indices

        def conv3x3_128(i, cout128=False):
            """layer i is 3x3 / stride 1 / pad 1 on 128 input channels, no depth-to-space, Cout a multiple of 128 (cout128: exactly 128)"""
            w = self.ws[i]
            return (tuple(w.shape[1:]) == (128, 3, 3) and (w.shape[0] == 128 if cout128 else w.shape[0] % 128 == 0)
                    and self.cfgs[i] == ([1, 1], [1, 1]) and self.ups[i] == 1)
        # the convs the live-tile machinery serves: layers 0 .. n-1, 2 <= n <= 8, all 128 -> 128 (0: none)
        live_convs = len(convs) if (convs == list(range(len(convs))) and 2 <= len(convs) <= 8
                                    and all(conv3x3_128(i, cout128=True) for i in convs)) else 0
        wl = self.ws[-1]
        deblock_1x1_128 = tuple(wl.shape) == (128, 128, 1, 1) and self.cfgs[-1] == ([1, 1], [0, 0]) and self.ups[-1] == 1
        # hand-written MFMA conv (sec_conv2d_nhwc, bias + ReLU fused) when shapes allow
        self.return_views = True   # the fused predict kernels read the head output in place through strides
        self.use_hip = backend == "hip" and dtype in (torch.bfloat16, torch.float16)
        self.packed, self.head_packed, self.head_b64, self.head_cout = [], None, None, 0
        if self.use_hip:
            for w in self.ws:
                pk = ops.conv2d_pack_weight(w.detach().contiguous())
                if pk is None:
                    self.use_hip = False
                    break
                self.packed.append(pk)
        if self.use_hip:
            self.head_cout = hw.shape[0] + (-hw.shape[0]) % 64
            hw64, self.head_b64 = self._padded_heads(self.head_cout)
            self.head_packed = ops.conv2d_pack_weight(hw64.to(dtype))
            self.use_hip = self.head_packed is not None
        # fp32 networks: every 3x3 / s1 / p1 128 -> Cout conv of a single-block RPN on the matrix pipe in one of two arithmetics.
        # backend "hip" with dtype float32 (the reference's default precision): split bf16 operands ("bf16x3").  backend "hip_f32" (the
        # exact mode's RPN, prepare_inference(exact_rpn="hip")): IEEE fp32 products on the fp32 MFMA.  Shapes the kernels do not take
        # keep the torch path.
        self.fp32, self.fp32_packed, self.fp32_chain = None, {}, None
        if backend == "hip_f32":
            assert dtype == torch.float32, "RPNInference(backend='hip_f32') is the fp32 form"
        arith = _FP32 if backend == "hip_f32" else _BF16X3 if (backend == "hip" and dtype == torch.float32) else None
        if arith is not None and single and next(rpn.parameters()).is_cuda and all(conv3x3_128(i) for i in convs):
            pk, chain = {i: arith.pack(self.ws[i]) for i in convs}, None
            # the 1x1 deblock + merged heads as ONE launch (sec_conv1x1_chain_x3 / _f32) when the shapes allow; otherwise they stay
            # torch fp32 GEMMs (9 GFLOP against the blocks' 500)
            if self.plan[-1][0] == "u" and deblock_1x1_128 and hw.shape[0] <= 64:
                hw64, hb64 = self._padded_heads(64)
                chain = [arith.pack(wl), arith.pack(hw64), hb64]
            if all(t is not None for t in list(pk.values()) + (chain or [])):
                self.fp32, self.fp32_packed, self.fp32_chain = arith, pk, chain
        self.concat_in_place = True      # multi-block RPNs: the deblocks write into the concatenated map (False: torch.cat of their outputs)
        self.pillar_rows_first = True    # a PillarBEV input: the first conv reads the pillar rows through a site map when the shapes allow (False: the scattered canvas)
        self.sparse_input = True   # forward()'s input comes from SparseConvTensor.dense(): all-zero halo tiles skip their MFMA loop (bit-identical)
        # first conv straight from the sparse rows (sec_conv2d_nhwc_gather): 3x3 / s1 / p1 on 2 planes x 64 channels; its weights
        # are packed a second time with the input channels in plane-major order (gather_first=False: always the dense image)
        self.gather_packed = None
        if self.use_hip and self.plan[0][0] == "c" and conv3x3_128(0) and gather_first:
            perm = ops.gather_channel_perm(64, 2).to(self.ws[0].device)
            self.gather_packed = ops.conv2d_pack_weight(self.ws[0].detach()[:, perm].contiguous())
        # deblock (1x1, stride 1, 128 -> 128) + heads (<= 128 padded channels) run as ONE kernel (sec_conv1x1_chain_nhwc)
        self.chain_tail = single and self.use_hip and deblock_1x1_128 and self.head_cout in (64, 128)
        # Background tiles (sec_conv2d_nhwc_tiles): with the first conv gathered from the sparse rows the site map is at hand, and a
        # tile of conv j's output that no site can reach (j + 1 steps) holds exactly what the network computes for an EMPTY frame at
        # that position -- any weights.  The empty frame's activations are computed once per map size by the
        # same kernels (:meth:`empty_frame_maps`); the convs then compute only the reachable tiles and copy the others.
        # skip_background = False convolves every tile.
        self.skip_background = True
        # lazy_background: the convs write their live tiles only and read their input's background tiles from the previous layer's
        # empty-frame map (sec_conv2d_nhwc_tiles_lazy) -- no copy of the ~1 450 background tiles (47 MB read + 47 MB written) per layer;
        # the fused 1x1 tail then runs on the last conv's lists whatever the live share (x_live_only)
        self.lazy_background = True
        # lazy_heads (set by SecondDetector around forwards whose consumer is the fused predict): the fused 1x1 tail writes the head
        # tensor's live tiles ONLY and the select / decode kernels read every other tile from the empty frame's head map -- the copy
        # of ~60 % of the [B, H, W, 64] head tensor (22 MB per batch of 8) disappears; forward() then adds preds["lazy_heads"]
        self.lazy_heads = False
        # fused_tail: with lazy heads the last 3x3 conv runs the 1x1 tail in its epilogue (sec_conv2d_nhwc_tiles_tail): one launch less, the
        # conv's output never reaches memory
        self.fused_tail = True
        self.last_live_counts = None       # [convs, B] int32 on the device: live tiles per conv and frame of the last forward (bench / tests)
        self.last_tiles_per_frame = None   # tiles of one frame's map in that forward
        # tile_cover: the single-block lazy chain with lazy heads and the fused tail follows COVER lists -- per 8-row band the reachable pixels
        # covered by tiles at free x (sec_rpn_tile_cover: 12 % fewer tiles than the fixed grid has live ones on the KITTI-like clouds);
        # every other path keeps the grid lists.  preds["lazy_heads"][0] is then the last conv's coverage (int32 words, a bit per pixel
        # column and band) instead of the per-tile flags, and the head tensor has holes INSIDE grid tiles: off for direct callers, set by
        # SecondDetector.lazy_heads(cover=True) around forwards whose preds go straight to the fused predict.  SEC_RPN_TILE_COVER=0|1
        # overrides (A/B, bit-identical detections).  last_live_counts stays the GRID's.
        self.tile_cover = False
        self.last_cover_counts = None      # [convs, B] int32: tiles per conv and frame of the cover lists, when the last forward followed them
        self._empty_maps = {}
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._repack())
        # (the fp32 forms: the same live-tile machinery on the split-operand / fp32-MFMA convs, always lazy)
        self.background_convs = live_convs if (self.gather_packed is not None or self.fp32 is not None) else 0

    def _padded_heads(self, cout):
        """(weight, bias) of the merged heads in fp32, zero-padded to ``cout`` output channels: the last GEMM of the fused 1x1 tails."""
        hw, hb = self.head_w.detach().float(), self.head_b.detach().float()
        pad = cout - hw.shape[0]
        return (torch.cat([hw, torch.zeros(pad, *hw.shape[1:], device=hw.device)], 0).contiguous(),
                torch.cat([hb, torch.zeros(pad, device=hb.device)]).contiguous())

    # The packed weight images (MFMA slab order, the gather permutation, the hi | lo pairs of the fp32 form) are derived from the
    # folded parameters at construction: keep them in step with the parameters.  In place, so that captured graphs stay valid.
    def _repack(self):
        with torch.no_grad():
            if self.use_hip:
                for i, w in enumerate(self.ws):
                    self.packed[i].copy_(ops.conv2d_pack_weight(w.detach().contiguous()))
                hw64, hb64 = self._padded_heads(self.head_cout)
                self.head_packed.copy_(ops.conv2d_pack_weight(hw64.to(self.head_w.dtype)))
                self.head_b64.copy_(hb64)
                if self.gather_packed is not None:
                    perm = ops.gather_channel_perm(64, 2).to(self.ws[0].device)
                    self.gather_packed.copy_(ops.conv2d_pack_weight(self.ws[0].detach()[:, perm].contiguous()))
            if self.fp32 is not None:
                for i, pk in self.fp32_packed.items():
                    pk.copy_(self.fp32.pack(self.ws[i]))
                if self.fp32_chain is not None:
                    hw64, hb64 = self._padded_heads(64)
                    for dst, src in zip(self.fp32_chain, (self.fp32.pack(self.ws[-1]), self.fp32.pack(hw64), hb64)):
                        dst.copy_(src)
        self._empty_maps.clear()

    def _apply(self, fn, *a, **k):
        super()._apply(fn, *a, **k)
        move = lambda t: fn(t) if isinstance(t, torch.Tensor) else t
        self.packed = [move(t) for t in self.packed]
        self.head_packed, self.head_b64, self.gather_packed = move(self.head_packed), move(self.head_b64), move(self.gather_packed)
        self.fp32_packed = {i: move(t) for i, t in self.fp32_packed.items()}
        if self.fp32_chain is not None:
            self.fp32_chain = [move(t) for t in self.fp32_chain]
        self._empty_maps.clear()
        return self

    def empty_frame_maps(self, h, w):
        """Output of every 3x3 conv of the block for a frame WITHOUT sites, channels_last [1, 128, h, w] each, from the kernels the
        forward itself uses (so that a copied tile is bit-identical to a computed one).  Cached per map size; the first call for a
        size must not happen inside a graph capture."""
        # keyed on the folded weights too (version counters, storage, device, dtype): load_state_dict into a prepared detector,
        # .to(device) or a dtype change must not leave maps of the old network behind (they fill every background tile)
        src = [self.ws[i] for i in range(self.background_convs)] + [self.bs[i] for i in range(self.background_convs)] + [self.ws[-1], self.bs[-1], self.head_w, self.head_b]
        key = (int(h), int(w), str(self.ws[0].device), self.ws[0].dtype, tuple((t.data_ptr(), t._version) for t in src))
        if key not in self._empty_maps:
            self._empty_maps.clear()
            assert not torch.cuda.is_current_stream_capturing(), "RPNInference.empty_frame_maps: run one eager forward before capturing"
            dev, dt = self.ws[0].device, self.ws[0].dtype
            with torch.no_grad():
                feat = torch.zeros((1, 64), dtype=dt, device=dev)
                sm = torch.zeros((1, 2, h, w), dtype=torch.int32, device=dev)
                x = ops.conv2d_nhwc_gather(feat, sm, self.gather_packed, self.bs[0], 128, relu=True)
                maps = [x]
                for i in range(1, self.background_convs):
                    x = ops.conv2d_nhwc(x, self.packed[i], self.bs[i], 128, 3, 1, 1, relu=True)
                    maps.append(x)
                if self.chain_tail:      # the fused deblock + heads on the empty frame: background of the tail
                    maps.append(ops.conv1x1_chain(x, self.packed[-1], self.bs[-1], self.head_packed, self.head_b64, self.head_cout))
            self._empty_maps[key] = maps
        return self._empty_maps[key]

    @staticmethod
    def _conv1x1_gemm(x, w, b, relu):
        """1x1 / stride 1 conv of a channels_last fp32 map as ONE GEMM over its [pixels, Cin] matrix (a view), bias in the GEMM's
        epilogue: MIOpen's fp32 1x1 convolution of the RPN tail (deblock 128 -> 128, heads 128 -> 64) ran as a grouped-conv kernel
        plus layout transposes, ~430 us per batch of 8 for 14 GFLOP."""
        n, c, h, wd = x.shape
        x2 = x.permute(0, 2, 3, 1).reshape(n * h * wd, c)                        # a view of the channels_last tensor
        y2 = torch.addmm(b.to(x2.dtype), x2, w.reshape(w.shape[0], c).t().to(x2.dtype))
        if relu:
            y2 = torch.relu_(y2)
        return y2.view(n, h, wd, w.shape[0]).permute(0, 3, 1, 2)                 # channels_last [n, cout, h, w]

    def _conv(self, x, i, sparse_input=False):
        w, b, (s, p) = self.ws[i], self.bs[i], self.cfgs[i]
        if self.use_hip:
            y = ops.conv2d_nhwc(x, self.packed[i], b, w.shape[0], w.shape[2], s[0], p[0], relu=True,
                                sparse_input=sparse_input)
        elif (x.dtype == torch.float32 and x.is_cuda and tuple(w.shape[2:]) == (1, 1) and s == [1, 1] and p == [0, 0]
              and x.is_contiguous(memory_format=torch.channels_last)):
            y = self._conv1x1_gemm(x, w, b, relu=True)
        else:
            y = ops.bias_act_(F.conv2d(x, w, None, s, p), b, relu=True)
        u = self.ups[i]
        if u > 1:   # depth-to-space of the channels-last result: [B,H,W,(dy,dx,co)] -> [B,H*u,W*u,co]
            n, c, h, wd = y.shape
            co = c // (u * u)
            y = y.permute(0, 2, 3, 1).reshape(n, h, wd, u, u * co).permute(0, 1, 3, 2, 4).reshape(n, h * u, wd * u, co)
            y = y.permute(0, 3, 1, 2)        # a channels_last [B,co,H*u,W*u] tensor
        return y

    def empty_frame_maps_fp32(self, h, w):
        """Output of every 3x3 conv of the fp32 forms for a frame WITHOUT sites, in the arithmetic's representation ((hi, lo) plane pairs
        or fp32 maps, channels_last [1, 128, h, w]), from the forward's own kernel (a copied or lazily read tile is then bit-identical
        to a computed one).  Cached per map size and weight version; not inside a capture."""
        src = [self.ws[i] for i in self.fp32_packed] + [self.bs[i] for i in self.fp32_packed]
        key = (self.fp32.name, int(h), int(w), str(self.ws[0].device), tuple((t.data_ptr(), t._version) for t in src))
        if key not in self._empty_maps:
            assert not torch.cuda.is_current_stream_capturing(), "RPNInference.empty_frame_maps_fp32: run one eager forward before capturing"
            self._empty_maps.clear()
            with torch.no_grad():
                a, maps = self.fp32.zeros(h, w, self.ws[0].device), []
                for i, pk in self.fp32_packed.items():
                    a = self.fp32.conv(a, pk, self.bs[i], self.ws[i].shape[0])
                    maps.append(a)
            self._empty_maps[key] = maps
        return self._empty_maps[key]

    def _forward_fp32(self, x):
        """The single block in one of the fp32 arithmetics (``self.fp32``).  Given the sparse middle's rows (a SparseBEV) the convs run on
        the tiles a site can reach only, exactly like the 16-bit path: conv j computes the tiles within j + 1 steps of a site, reads
        halo pixels of unwritten tiles from the empty frame's maps, and only the last conv materialises its background, because the
        1x1 tail (deblock + heads: one launch, or torch fp32 GEMMs on the map merged back to fp32) reads the whole map."""
        ar, lists = self.fp32, None
        if isinstance(x, SparseBEV):
            if self.background_convs and self.skip_background:
                sm = x.site_map()
                empty = self.empty_frame_maps_fp32(sm.shape[2], sm.shape[3])
                live, self.last_live_counts, nbr = x.tile_lists(self.background_convs, masks=True)
                lists = (live, nbr, empty)
            x = x.dense()
        a = ar.enter(x.float().contiguous(memory_format=torch.channels_last))
        first = self.sparse_input
        for i, pk in self.fp32_packed.items():
            if lists is not None:
                live, nbr, empty = lists
                last = i == self.background_convs - 1
                a = ar.conv_tiles(a, pk, self.bs[i], self.ws[i].shape[0], live[i], self.last_live_counts[i],
                                  background=empty[i] if last else None, nbr_masks=nbr[i] if i > 0 else None,
                                  background_in=empty[i - 1] if i > 0 else None)
            else:
                a = ar.conv(a, pk, self.bs[i], self.ws[i].shape[0], sparse_input=first)
                first = False
        i = len(self.ws) - 1                       # the one deblock of the single block
        if self.fp32_chain is not None:
            w1, w2, b2 = self.fp32_chain
            return self._split_heads(ar.chain(a, w1, self.bs[i], w2, b2))
        f = self._conv(ar.leave(a), i)
        if f.is_cuda and f.is_contiguous(memory_format=torch.channels_last):
            y = self._conv1x1_gemm(f, self.head_w, self.head_b, relu=False)
        else:
            y = ops.bias_act_(F.conv2d(f, self.head_w, None), self.head_b, relu=False)
        return self._split_heads(y)

    def _split_heads(self, y):
        n, _, h, wd = y.shape
        ret, c0 = {}, 0
        for name, sz, code in zip(["box_preds", "cls_preds", "dir_cls_preds"], self.splits, self.codes):
            o = y[:, c0:c0 + sz]
            c0 += sz
            o = o.reshape(n, self.a, code, h, wd).permute(0, 1, 3, 4, 2)   # [B,A,H,W,code] view of the head output
            ret[name] = o if self.return_views else o.contiguous()
        return ret

    def forward(self, x):
        if self.fp32 is not None:
            return self._forward_fp32(x.dense() if isinstance(x, PillarBEV) else x)
        ups = []
        first = self.sparse_input     # x is the scattered sparse-middle output: mostly empty tiles
        gather = None
        if isinstance(x, SparseBEV):
            if self.gather_packed is not None:
                gather = x
            else:
                x = x.dense()
        if isinstance(x, PillarBEV):
            kind0, i0 = self.plan[0]
            w0, (s0, p0) = self.ws[i0], self.cfgs[i0]
            if (self.use_hip and self.pillar_rows_first and kind0 == "c" and x.features.dtype == w0.dtype and w0.shape[2] == w0.shape[3]
                    and ops.conv2d_rows_supported(x.features.shape[1], w0.shape[0], w0.shape[2], s0[0], p0[0], w0.dtype) and w0.shape[1] == x.features.shape[1]):
                pillars, x = x, None
            else:
                x = x.dense()
        else:
            pillars = None
        live = nbr = cover = fused_heads = stage0 = None
        catbuf, coff = None, 0
        for kind, i in self.plan:
            if self.stage0_layer is not None and i == self.stage0_layer + 1:
                stage0 = x               # layers run in index order: the output of layer ``stage0_layer``
            if kind == "c" and x is None:
                # the first conv straight from the pillar rows (sec_conv2d_nhwc_rows): no zero fill, no scatter, no 82 MB canvas
                x = ops.conv2d_nhwc_rows(pillars.features, pillars.site_map(), self.packed[i], self.bs[i], self.ws[i].shape[0],
                                         self.ws[i].shape[2], self.cfgs[i][0][0], self.cfgs[i][1][0], relu=True)
                first = False
            elif kind == "c" and gather is not None:
                sm = gather.site_map()
                if self.background_convs and self.skip_background:
                    empty = self.empty_frame_maps(sm.shape[2], sm.shape[3])
                    lazy = self.lazy_background and self.background_convs >= 2
                    layers_, masks_, cover_ = self.tile_list_request(sm.shape[2], sm.shape[3])
                    if cover_:
                        live, self.last_live_counts, cover = gather.tile_lists(layers_, cover=True)
                        self.last_cover_counts = cover.counts
                    elif lazy:
                        live, self.last_live_counts, nbr = gather.tile_lists(layers_, masks=True)
                    else:
                        (live, self.last_live_counts), nbr = gather.tile_lists(layers_), None
                    self.last_tiles_per_frame = int(live.shape[-1])
                    if cover is not None:
                        x = ops.conv2d_nhwc_gather(gather.features, sm, self.gather_packed, self.bs[i], self.ws[i].shape[0], relu=True,
                                                   tile_order=cover.order[0], live_counts=cover.counts[0], cover=True)
                    else:
                        self.last_cover_counts = None
                        x = ops.conv2d_nhwc_gather(gather.features, sm, self.gather_packed, self.bs[i], self.ws[i].shape[0], relu=True,
                                                   tile_order=live[0], live_counts=self.last_live_counts[0], background=None if lazy else empty[0])
                else:
                    x = ops.conv2d_nhwc_gather(gather.features, sm, self.gather_packed, self.bs[i], self.ws[i].shape[0], relu=True)
                gather, first = None, False
            elif kind == "c" and cover is not None and i == self.background_convs - 1:
                # the cover form of the chain ends in the fused tail (tile_list_request): sec_conv2d_nhwc_tiles_tail_cover
                fused_heads = ops.conv2d_nhwc_tiles_tail(x, self.packed[i], self.bs[i], cover.order[i], cover.counts[i], None, empty[i - 1],
                                                         self.packed[-1], self.bs[-1], self.head_packed, self.head_b64, self.head_cout,
                                                         cover_halo=cover.halo[i])
                x = None
            elif kind == "c" and cover is not None:
                x = ops.conv2d_nhwc_tiles(x, self.packed[i], self.bs[i], 128, cover.order[i], cover.counts[i], None, relu=True,
                                          cover_halo=cover.halo[i], background_in=empty[i - 1])
            elif kind == "c" and live is not None and nbr is not None and self._tail_in_last_conv(i, x, nbr):
                # the last conv with the 1x1 tail (deblock + heads) in its epilogue: its output tile never leaves LDS (sec_conv2d_nhwc_tiles_tail)
                fused_heads = ops.conv2d_nhwc_tiles_tail(x, self.packed[i], self.bs[i], live[i], self.last_live_counts[i], nbr[i], empty[i - 1],
                                                         self.packed[-1], self.bs[-1], self.head_packed, self.head_b64, self.head_cout)
                x = None
            elif kind == "c" and live is not None and nbr is not None:
                # the last conv keeps its copies unless its consumer is the fused 1x1 tail on the same lists (x_live_only below)
                keep = i == self.background_convs - 1 and not self.chain_tail
                x = ops.conv2d_nhwc_tiles(x, self.packed[i], self.bs[i], 128, live[i], self.last_live_counts[i], empty[i] if keep else None,
                                          relu=True, nbr_masks=nbr[i], background_in=empty[i - 1])
            elif kind == "c" and live is not None:
                x = ops.conv2d_nhwc_tiles(x, self.packed[i], self.bs[i], 128, live[i], self.last_live_counts[i], empty[i], relu=True)
            elif kind == "c":
                x = self._conv(x, i, sparse_input=first)
                first = False
            elif self.chain_tail:
                ups.append(None)                     # single block: the deblock runs fused with the heads below
            elif self._deblocks_write_into_the_concat():
                # multi-block RPN: every deblock deposits its channels straight into the map the heads read (no torch.cat; sec_conv2d_nhwc_into)
                w_, (s_, p_) = self.ws[i], self.cfgs[i]
                if catbuf is None:
                    ho, wo = (x.shape[2] + 2 * p_[0] - w_.shape[2]) // s_[0] + 1, (x.shape[3] + 2 * p_[1] - w_.shape[3]) // s_[1] + 1
                    catbuf = torch.empty((x.shape[0], self._cat_channels, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
                    coff = 0
                ups.append(ops.conv2d_nhwc_into(x, self.packed[i], self.bs[i], w_.shape[0], w_.shape[2], s_[0], p_[0], True, catbuf, coff))
                coff += w_.shape[0]
            else:
                ups.append(self._conv(x, i))
        lazy_heads = None
        if fused_heads is not None and cover is not None:     # "written" = the last conv's coverage, a bit per pixel column and band
            y = fused_heads
            lazy_heads = (cover.cols[self.background_convs - 1], self._split_heads(empty[self.background_convs]))
        elif fused_heads is not None:
            y = fused_heads
            lazy_heads = (nbr[self.background_convs, 1], self._split_heads(empty[self.background_convs]))
        elif self.chain_tail and live is not None:
            last = self.background_convs - 1
            want_lazy = self.lazy_heads and nbr is not None and nbr.shape[0] > self.background_convs
            y = ops.conv1x1_chain(x, self.packed[-1], self.bs[-1], self.head_packed, self.head_b64, self.head_cout,
                                  tile_order=live[last], live_counts=self.last_live_counts[last],
                                  background=None if want_lazy else empty[last + 1], x_live_only=nbr is not None)
            if want_lazy:      # (tile-indexed masks of the layer BEHIND the last conv: bit 4 = the last conv's list holds the tile)
                lazy_heads = (nbr[self.background_convs, 1], self._split_heads(empty[last + 1]))
        elif self.chain_tail:
            y = ops.conv1x1_chain(x, self.packed[-1], self.bs[-1], self.head_packed, self.head_b64, self.head_cout)
        else:
            f = catbuf if catbuf is not None else (x if not ups else ups[0] if len(ups) == 1 else torch.cat(ups, dim=1))    # channels_last in, channels_last out
            if self.use_hip:
                y = ops.conv2d_nhwc(f.contiguous(memory_format=torch.channels_last), self.head_packed, self.head_b64,
                                    self.head_cout, 1, 1, 0, relu=False)
            else:
                y = ops.bias_act_(F.conv2d(f, self.head_w, None), self.head_b, relu=False)
        ret = self._split_heads(y)
        if lazy_heads is not None:
            ret["lazy_heads"] = lazy_heads          # consumed by SecondDetector._predict_fused (ops.predict_select / predict_decode lazy=)
        if stage0 is not None:
            ret["stage0"] = stage0
        return ret

    def _tail_in_last_conv(self, i, x, nbr):
        """Conv ``i`` is the last 3x3 conv of a single-block RPN whose consumers are all lazy (lazy heads on the same lists): it then runs
        with the 1x1 tail in its epilogue.  SEC_RPN_FUSED_TAIL=0: the two launches (A/B, bit-identical)."""
        return (self.fused_tail and i == self.background_convs - 1 and self.chain_tail and self.lazy_heads and self.head_cout == 64
                and nbr.shape[0] > self.background_convs and x is not None and x.shape[1] == 128
                and x.dtype in (torch.bfloat16, torch.float16) and os.environ.get("SEC_RPN_FUSED_TAIL", "1") != "0")

    def _deblocks_write_into_the_concat(self):
        """Several deblocks, each a plain conv (no depth-to-space) of a shape sec_conv2d_nhwc_into serves: they fill one preallocated map."""
        v = getattr(self, "_into_ok", None)
        if v is None:
            us = [i for kind, i in self.plan if kind == "u"]
            v = bool(self.use_hip and self.concat_in_place and len(us) > 1 and all(
                self.ups[i] == 1 and self.cfgs[i][0][0] == self.cfgs[i][0][1] and self.cfgs[i][1][0] == self.cfgs[i][1][1] and self.ws[i].shape[2] == self.ws[i].shape[3]
                and ops.conv2d_into_supported(self.ws[i].shape[1], self.ws[i].shape[0], self.ws[i].shape[2], self.cfgs[i][0][0], self.cfgs[i][1][0], self.ws[i].dtype)
                for i in us))
            self._cat_channels = sum(self.ws[i].shape[0] for i in us)
            self._into_ok = v
        return v

    def tile_list_request(self, h, w):
        """(layers, masks, cover) a forward on an h x w map passes to SparseBEV.tile_lists -- a staged capture asks for the same lists ahead
        of the RPN segment.  cover: the single-block lazy chain (128 -> 128 convs, 16-bit) whose last conv runs the fused tail for lazy heads
        (the condition of :meth:`_tail_in_last_conv`) on a map whose cover entries fit 16 bits; SEC_RPN_TILE_COVER=0|1 forces the grid lists /
        the cover lists wherever that chain runs."""
        lazy = self.lazy_background and self.background_convs >= 2
        env = os.environ.get("SEC_RPN_TILE_COVER", "")
        want = self.tile_cover if env not in ("0", "1") else env == "1"
        n = self.background_convs
        chain = (lazy and self.fused_tail and self.chain_tail and self.lazy_heads and self.head_cout == 64 and n < 8
                 and sum(1 for kind, _ in self.plan if kind == "c") == n and all(tuple(self.ws[j].shape[:2]) == (128, 128) for j in range(n))
                 and self.ws[0].dtype in (torch.bfloat16, torch.float16) and os.environ.get("SEC_RPN_FUSED_TAIL", "1") != "0")
        if want and chain and ops.rpn_tile_cover_supported(h, w, n):
            return n, False, True
        return (self.list_layers(), True, False) if lazy else (n, False, False)

    def list_layers(self):
        """Layers of live-tile lists / masks a forward asks rpn_tile_live for: one per 3x3 conv, plus one when the heads are lazy (its
        tile-indexed masks say which tiles the LAST conv's list -- the fused tail's -- holds)."""
        return self.background_convs + (1 if (self.lazy_heads and self.chain_tail and self.background_convs < 8) else 0)


class _TrunkAsRPN(nn.Module):
    """An RPNNoHead trunk with a DefaultHead's three convs, presented to RPNInference as the RPNV2 it folds and packs."""

    def __init__(self, trunk, head):
        super().__init__()
        self.blocks, self.deblocks, self._upsample_start_idx = trunk.blocks, trunk.deblocks, trunk._upsample_start_idx
        self.conv_box, self.conv_cls = head.conv_box, head.conv_cls
        self._num_anchor_per_loc, self._num_class, self._box_code_size = head._num_anchor_per_loc, head._num_class, head._box_code_size
        self._num_direction_bins, self._use_direction_classifier = head._num_direction_bins, head._use_direction_classifier
        if head._use_direction_classifier:
            self.conv_dir_cls = head.conv_dir_cls


class _TowerAsRPN(_TrunkAsRPN):
    """A SmallObjectHead the same way: its tower is the one block, the heads read that block's output (no deblock)."""

    _heads_on_last_block = True

    def __init__(self, head):
        nn.Module.__init__(self)
        self.blocks, self.deblocks, self._upsample_start_idx = nn.ModuleList([head.net]), nn.ModuleList(), 1
        self.conv_box, self.conv_cls = head.conv_box, head.conv_cls
        self._num_anchor_per_loc, self._num_class, self._box_code_size = head._num_anchor_per_loc, head._num_class, head._box_code_size
        self._num_direction_bins, self._use_direction_classifier = head._num_direction_bins, head._use_direction_classifier
        if head._use_direction_classifier:
            self.conv_dir_cls = head.conv_dir_cls


class MultiHeadInference(nn.Module):
    """Inference form of the multi-head network's dense part (net_multi_head.py:150-176): two RPNInference plans.  ``trunk`` = the
    RPNNoHead blocks / deblocks with the large head's 1x1 convs on the concatenated map, which also hands out block 0's output;
    ``tower`` = the small head's three 3x3 convs (BatchNorm folded with the module's own eps, 1e-5) and its 1x1 convs on the crop of
    that output.  The crop is COPIED to a tensor of its own: the tower's first conv zero-pads at the crop's border, as the
    reference's does on its slice, and never sees the stage-0 cells outside it.
    Returns {"box_preds", "cls_preds", "dir_cls_preds"}, each a LIST of [B, A_s, H_s, W_s, code] views, large head first -- the
    order the reference concatenates in and ops.predict_select / predict_decode take."""

    def __init__(self, trunk, large_head, small_head, dtype, backend="hip"):
        super().__init__()
        self.trunk = RPNInference(_TrunkAsRPN(trunk, large_head), dtype, backend=backend, gather_first=False)
        self.trunk.stage0_layer = self.trunk.block_last[0]
        self.tower = RPNInference(_TowerAsRPN(small_head), dtype, backend=backend, gather_first=False)
        self.tower.sparse_input = False

    @property
    def use_hip(self):
        return self.trunk.use_hip and self.tower.use_hip

    def small_head_of(self, stage0):
        """The small head's predictions from block 0's output: the crop as a tensor of its own, then the tower."""
        c = stage0_crop(stage0.shape[2])
        return self.tower(stage0[:, :, c:-c, c:-c].contiguous(memory_format=torch.channels_last))

    def forward(self, x):
        large = self.trunk(x)
        small = self.small_head_of(large.pop("stage0"))
        return {k: [large[k], small[k]] for k in large}


def flat_preds(preds, batch_size):
    """Prediction tensors as the reference's [B, N, code] (net_multi_head.py:170-176): lists of per-head views are flattened and
    concatenated in order; anything else passes."""
    return {k: (torch.cat([t.reshape(batch_size, -1, t.shape[-1]) for t in v], 1) if isinstance(v, (list, tuple)) else v)
            for k, v in preds.items()}


# ------------------------------------------------------------------------------------------ detector
def limit_period(val, offset, period):
    return val - torch.floor(val / period + offset) * period


class SecondDetector(nn.Module):
    """VoxelNet mirror.  ``forward(example)`` accepts the reference's example dict
    (voxels, num_points, coordinates, anchors; voxelnet.py:339-375) and returns the reference's list of
    prediction dicts; ``forward_points`` is the device-resident fast path (raw clouds in, detections out,
    no host sync until the caller reads the result)."""

    box_ndim = 7        # values per box row; __init__ sets 7 + the config's custom values

    def __init__(self, cfg=CAR_FHD):
        super().__init__()
        self.cfg = cfg
        gs = grid_size_of(cfg)
        self.grid_size = gs
        dense_shape = [1] + gs[::-1].tolist() + [64]
        self.pillars = cfg.get("vfe") in PILLAR_VFES
        self.encoder = "SimpleVoxelRadius" if cfg.get("vfe") == "SimpleVoxelRadius" else "SimpleVoxel"
        if self.pillars:
            self.voxel_feature_extractor = VFES[cfg["vfe"]](cfg["num_point_features"], cfg["vfe_filters"], cfg["voxel_size"],
                                                            cfg["point_cloud_range"],
                                                            with_distance=bool(cfg.get("vfe_with_distance", False)))
            self.middle_feature_extractor = PointPillarsScatter(dense_shape, cfg["middle_in"])
        else:
            self.voxel_feature_extractor = VFES[cfg.get("vfe", "SimpleVoxel")](cfg["num_point_features"])
            self.middle_feature_extractor = MIDDLES[cfg.get("middle", "SpMiddleFHD")](dense_shape, cfg["middle_in"])
            if cfg["middle_in"] < 4 and isinstance(self.middle_feature_extractor, SpMiddleFHD):
                self.middle_feature_extractor.middle_conv[0].pad_in_channels = 4      # KITTI all.fhd: SubMConv3d(3, 16) on radius rows
        # a config adopted from a reference-built VoxelNet (second_amd.dropin) names the anchor count only: its anchors arrive
        # with every example (voxelnet.py:358), so no anchor table is generated here
        a_per_loc = int(cfg.get("num_anchor_per_loc") or (sum(h["num_anchor_per_loc"] for h in cfg["heads"]) if cfg.get("heads")
                                                          else anchors_per_location(cfg)))
        self.num_anchor_per_loc = a_per_loc
        fm = [1, int(gs[1]) // cfg["downsample_factor"], int(gs[0]) // cfg["downsample_factor"]]
        self.feature_map_size = fm
        self.box_ndim = box_ndim_of(cfg)       # 7 + custom values (nuScenes velocity: 9): the heads' box_code_size, every box row's width
        if self.box_ndim != 7 and cfg.get("multiclass_nms"):
            raise ValueError(f"{cfg['name']}: multiclass_nms with anchor_custom_values is not supported (the multi-class NMS chain "
                             f"serves box rows of 7 values)")
        self.heads = cfg.get("heads")          # multi-head networks (VoxelNetNuscenesMultiHead): [large_head on "out", small_head on "stage0"]
        if self.heads:
            self._check_heads(cfg, fm)
            self.rpn = RPNNoHead(num_class=cfg["num_class"], num_direction_bins=cfg["num_direction_bins"], box_code_size=self.box_ndim,
                                 **cfg["rpn"])
            kw = dict(num_class=cfg["num_class"], num_direction_bins=cfg["num_direction_bins"], box_code_size=self.box_ndim,
                      use_direction_classifier=cfg["rpn"].get("use_direction_classifier", True))
            # at top level, as the reference has them (net_multi_head.py:131-148)
            self.small_head = SmallObjectHead(cfg["rpn"]["num_filters"][0], num_anchor_per_loc=self.heads[1]["num_anchor_per_loc"], **kw)
            self.large_head = DefaultHead(sum(cfg["rpn"]["num_upsample_filters"]), num_anchor_per_loc=self.heads[0]["num_anchor_per_loc"], **kw)
        else:
            self.rpn = RPNV2(num_class=cfg["num_class"], num_anchor_per_loc=a_per_loc, num_direction_bins=cfg["num_direction_bins"],
                             box_code_size=self.box_ndim, **cfg["rpn"])
        self.register_buffer("global_step", torch.LongTensor(1).zero_())
        if cfg.get("anchor_sizes"):
            self.register_buffer("anchors", torch.from_numpy(generate_anchors(cfg, fm)), persistent=False)
        else:
            self.anchors = None
        self.register_buffer("_arange_p", torch.arange(cfg["nms_post_max_size"], dtype=torch.int32), persistent=False)
        self.register_buffer("post_center_range", torch.tensor(cfg["post_center_range"], dtype=torch.float32),
                             persistent=False)
        self._infer_dtype = None
        self.pfn_slots = True        # PointPillars inference: the PillarFeatureNet walks the voxeliser's point lists (False: pillar tensor)
        self.fused_predict = True
        self.multiclass = multiclass_nms_settings(cfg, a_per_loc, fm)      # None unless cfg["multiclass_nms"]
        self.rulebook_numbering = os.environ.get("SEC_RULEBOOK_NUMBERING", "sorted")
        bf = cfg.get("block_filtering")
        self.voxel_generator = spconv.utils.VoxelGeneratorV2(cfg["voxel_size"], cfg["point_cloud_range"],
                                                            cfg["max_points_per_voxel"], cfg["max_voxels"],
                                                            **(dict(bf, block_filtering=True) if bf else {}))

    @staticmethod
    def _check_heads(cfg, fm):
        """A multi-head config this mirror reproduces: the large head on the trunk's concatenated map first, the small head on block 0's
        cropped output second -- the order net_multi_head.py:170-176 concatenates the predictions in -- and, when the config lists
        anchors, every anchor generator of the ``out`` map before every one of the ``stage0`` map, with matching counts."""
        heads = cfg["heads"]
        if [(h["name"], h["source"]) for h in heads] != [("large_head", "out"), ("small_head", "stage0")]:
            raise ValueError(f"{cfg['name']}: multi-head networks are [large_head on 'out', small_head on 'stage0'], got "
                             f"{[(h['name'], h['source']) for h in heads]}")
        if [int(v) for v in heads[0]["feature_map_size"]] != fm:
            raise ValueError(f"{cfg['name']}: large_head's feature_map_size {heads[0]['feature_map_size']} is not the trunk's map {fm}")
        if not cfg.get("anchor_sizes"):
            return
        groups = cfg.get("anchor_groups") or [[i] for i in range(len(cfg["anchor_sizes"]))]
        sizes = [group_feature_map_size(cfg, gi, fm) for gi in range(len(groups))]
        of_head = [0 if sz == [int(v) for v in heads[0]["feature_map_size"]] else 1 if sz == [int(v) for v in heads[1]["feature_map_size"]] else None
                   for sz in sizes]
        if None in of_head or of_head != sorted(of_head):
            raise ValueError(f"{cfg['name']}: class order: every class of the 'out' map ({heads[0]['feature_map_size']}) must precede every "
                             f"class of the 'stage0' map ({heads[1]['feature_map_size']}); the classes' maps are {sizes}")
        for hi, h in enumerate(heads):
            n = sum(len(g) * len(cfg.get("group_rotations", {}).get(gi, cfg["rotations"])) for gi, g in enumerate(groups) if of_head[gi] == hi)
            if n != h["num_anchor_per_loc"]:
                raise ValueError(f"{cfg['name']}: {h['name']} has {h['num_anchor_per_loc']} anchors per cell, its classes generate {n}")

    # -- inference preparation: bf16 channels-last RPN with folded BN; sparse stack in bf16 (BN folded at run time)
    def prepare_inference(self, dtype=torch.bfloat16, rpn_backend="hip", gather_first=True, exact=False, exact_rpn=None):
        """``dtype=torch.float32`` selects the fp32-STORAGE pipeline, whose products by default run as three bf16 MFMA passes on split
        operands (16 significant bits per operand, fp32 accumulation; reported as ``ops.FP32_SPLIT_LABEL`` = "bf16x3").  ``exact=True``:
        true fp32 arithmetic, the reference's default precision (train.py:232-235) -- sparse convs on v_mfma_f32_32x32x2_f32 / VALU
        (``ops.fp32_mode("exact")`` around every forward), the RPN on torch's fp32 convolutions: several times slower, for parity work.
        ``exact_rpn`` picks the exact mode's RPN: "torch" (those convolutions) or "hip" (``RPNInference(backend="hip_f32")``: the
        fp32-MFMA convs on live tiles, no vendor convolution); None = the process default, :func:`exact_rpn_default` (SEC_FP32_RPN)."""
        # NOTE: MIOpen's fused conv+bias+ReLU plan (torch.miopen_convolution_relu) was measured at ~160 ms per
        # 3x3 conv for bf16 NHWC on gfx950 (naive fallback kernel) vs 0.14 ms unfused -- not an option; the
        # fused dense path is the hand-written MFMA conv.
        self.eval()
        self.fp32_exact = bool(exact) and dtype == torch.float32
        if exact_rpn is not None and exact_rpn not in EXACT_RPN_BACKENDS:
            raise ValueError(f"exact_rpn={exact_rpn!r}: allowed values are 'torch' and 'hip'")
        if self.fp32_exact:
            rpn_backend = "hip_f32" if (exact_rpn or exact_rpn_default()) == "hip" else "miopen"
        if isinstance(self.rpn, RPNNoHead):
            if not (RPNInference.supports(self.rpn) and next(self.parameters()).is_cuda):
                raise NotImplementedError(f"{self.cfg['name']}: prepare_inference of a multi-head network needs the GPU and plain-conv deblocks")
            self.rpn = MultiHeadInference(self.rpn, self.large_head, self.small_head, dtype, backend=rpn_backend)
        elif isinstance(self.rpn, RPNV2) and RPNInference.supports(self.rpn) and next(self.parameters()).is_cuda:
            self.rpn = RPNInference(self.rpn, dtype, backend=rpn_backend, gather_first=gather_first)
        else:
            self.rpn.blocks = nn.ModuleList([fold_conv_bn_(b) for b in self.rpn.blocks])
            self.rpn.deblocks = nn.ModuleList([fold_conv_bn_(b) for b in self.rpn.deblocks])
            self.rpn.to(dtype).to(memory_format=torch.channels_last)
        for m in self.middle_feature_extractor.modules():
            if isinstance(m, spconv.SparseConvolution):
                m.weight.data = m.weight.data.to(dtype)
        self._infer_dtype = dtype
        return self

    # -- stages ------------------------------------------------------------------------------------
    def network_forward(self, voxel_features, coors, batch_size, num_active_dev=None, site_table=None, in_pitch=None):
        """``in_pitch``: see the sparse middle's forward (pitch-4 rows of SimpleVoxelRadius.rows4 / the voxeliser's radius epilogue)."""
        with ops.fp32_mode("exact" if getattr(self, "fp32_exact", False) else None):
            return self._network_forward(voxel_features, coors, batch_size, num_active_dev, site_table, in_pitch)

    def arithmetic(self):
        """What the prepared pipeline computes with, for records: "bf16" / "fp16" (16-bit features, fp32 accumulation), "fp32" (exact
        mode: IEEE fp32 products) or "bf16x3" (fp32 storage, split-operand products)."""
        dt = self._infer_dtype
        if dt in (torch.bfloat16, torch.float16):
            return "bf16" if dt == torch.bfloat16 else "fp16"
        if getattr(self, "fp32_exact", False) or (next(self.parameters()).is_cuda and ops.get_fp32_mode() == "exact"):
            return "fp32"
        return ops.FP32_SPLIT_LABEL if next(self.parameters()).is_cuda else "fp32"

    def _network_forward(self, voxel_features, coors, batch_size, num_active_dev=None, site_table=None, in_pitch=None):
        dt = self._infer_dtype
        pitch = {} if in_pitch is None else {"in_pitch": in_pitch}
        if self.pillars:
            mfe = self.middle_feature_extractor
            rows_rpn = self.rpn.trunk if isinstance(self.rpn, MultiHeadInference) else self.rpn
            if (dt in (torch.bfloat16, torch.float16) and isinstance(rows_rpn, RPNInference) and rows_rpn.use_hip and rows_rpn.fp32 is None
                    and isinstance(mfe, PointPillarsScatter) and not torch.is_grad_enabled()):
                # no canvas: the RPN's first conv gathers the pillar rows (PillarBEV.dense() is the scatter for the shapes it does not take)
                return self.rpn(PillarBEV(voxel_features.to(dt), coors, batch_size, mfe.ny, mfe.nx, num_dev=num_active_dev))
            spatial = mfe(voxel_features if dt is None else voxel_features.to(dt), coors,
                          batch_size, channels_last=dt is not None, num_dev=num_active_dev)
            if isinstance(self.rpn, RPNNoHead):
                return self.multi_head_dense(spatial)
            return self.rpn(spatial)
        if dt is not None:
            spatial = self.middle_feature_extractor(voxel_features.to(dt), coors, batch_size, channels_last=True,
                                                    num_active_dev=num_active_dev, site_table=site_table,
                                                    bev_sparse=self._rpn_takes_rows(), **pitch)
        else:
            spatial = self.middle_feature_extractor(voxel_features, coors, batch_size, num_active_dev=num_active_dev,
                                                    site_table=site_table, **pitch)
        return self.rpn(spatial)

    def multi_head_dense(self, spatial):
        """The module graph of the multi-head network behind the pseudo image (net_multi_head.py:150-176): trunk, small head on the
        cropped stage 0, large head on the concatenated map; predictions concatenated large first."""
        out = self.rpn(spatial)
        c = stage0_crop(out["stage0"].shape[2])
        small = self.small_head(out["stage0"][:, :, c:-c, c:-c])
        large = self.large_head(out["out"])
        return {k: torch.cat([large[k], small[k]], dim=1) for k in large}

    def _rpn_takes_rows(self):
        """The RPN consumes the sparse middle's rows + site map (SparseBEV) instead of the dense image: the 16-bit gathered first conv, or
        the fp32 split-operand / fp32-MFMA convs on live tiles."""
        return getattr(self.rpn, "gather_packed", None) is not None or (
            getattr(self.rpn, "fp32", None) is not None and getattr(self.rpn, "background_convs", 0) > 0)

    def forward(self, example):
        voxels, num_points, coors = example["voxels"], example["num_points"], example["coordinates"]
        batch_size = example["anchors"].shape[0]
        pitch = None
        if self.encoder == "SimpleVoxelRadius":      # (decided under the caller's grad mode: the pitch-4 rows are an inference form)
            feats, pitch = self.voxel_feature_extractor.encode(voxels, num_points)
        else:
            with torch.no_grad():
                feats = self.voxel_feature_extractor(voxels, num_points, coors)
        preds = self.network_forward(feats, coors, batch_size, in_pitch=pitch)
        with torch.no_grad():
            return self.predict(preds, example["anchors"].view(batch_size, -1, self.box_ndim), example.get("anchors_mask"))

    def forward_points(self, points, point_offsets, static=False):
        """points [N,4] cuda float32 (clouds concatenated), point_offsets [B+1] cuda int32.

        ``static=True``: static-capacity, sync-free pipeline (every buffer sized for N rows, live counts stay
        on the device) -- hipGraph-capturable; call :meth:`check_overflow` whenever the host next syncs.

        The strided rulebooks of this path use ``self.rulebook_numbering`` ("sorted" = spconv's GPU output numbering: no
        hash table; the row order is internal here -- the dense feature map and the detections are identical to the
        first-touch form; SEC_RULEBOOK_NUMBERING overrides)."""
        prev = ops.set_rulebook_numbering(self.rulebook_numbering)
        try:
            return self._forward_points(points, point_offsets, static)
        finally:
            ops.set_rulebook_numbering(prev)

    def lazy_heads(self, cover=False):
        """Context: forwards inside may leave the head tensor's background tiles unwritten (RPNInference.lazy_heads) because their
        preds go straight to :meth:`predict_device`'s fused kernels, which read those tiles from the empty frame's map.  A no-op when
        the prepared RPN / the predict path cannot do it (or SEC_RPN_LAZY_HEADS=0).  ``cover``: the RPN may also follow the cover lists
        (RPNInference.tile_cover: nobody but the fused predict looks at the head tensor, whose written region is then no union of grid tiles)."""
        det = self

        class _Ctx:
            def __enter__(self_):
                self_.prev = getattr(det.rpn, "lazy_heads", None)
                self_.prev_cover = getattr(det.rpn, "tile_cover", None)
                if (self_.prev is not None and det.fused_predict and det.cfg["nms_pre_max_size"] <= 1024 and det.multiclass is None
                        and os.environ.get("SEC_RPN_LAZY_HEADS", "1") != "0"):
                    det.rpn.lazy_heads = True
                    if cover and self_.prev_cover is not None:
                        det.rpn.tile_cover = True
                return self_

            def __exit__(self_, *exc):
                if self_.prev is not None:
                    det.rpn.lazy_heads = self_.prev
                if self_.prev_cover is not None:
                    det.rpn.tile_cover = self_.prev_cover
                return False
        return _Ctx()

    def _forward_points(self, points, point_offsets, static=False):
        with self.lazy_heads(cover=True):
            return self._forward_points_impl(points, point_offsets, static)

    def _forward_points_impl(self, points, point_offsets, static=False):
        batch_size = point_offsets.numel() - 1
        nf = self.cfg["num_point_features"]
        if self.pillars:
            # inference on 4-feature points: the PillarFeatureNet walks the voxeliser's point lists (no [P, 60, 4] tensor: 98 MB
            # written and re-read per step at nuScenes size); pfn_slots = False materialises the pillars as the reference does
            # (block filtering returns compacted pillars without the voxeliser's point lists: tensor path)
            slots = (not self.training and not torch.is_grad_enabled() and nf == 4 and points.shape[1] == 4 and points.is_cuda
                     and not getattr(self.voxel_generator, "_block_filtering", False)
                     and self.pfn_slots)
            vox = self.voxel_generator.generate_device(points, point_offsets, sync=not static, fill=not slots)
            nd = vox["voxel_offsets"][batch_size:] if static else None    # device count of live pillars
            if slots:
                feats = self.voxel_feature_extractor.forward_slots(points, vox, out_dtype=self._infer_dtype, num_dev=nd)
            else:
                feats = self.voxel_feature_extractor(vox["voxels"], vox["num_points_per_voxel"], vox["coordinates"],
                                                     out_dtype=self._infer_dtype, num_dev=nd)
            preds = self.network_forward(feats, vox["coordinates"], batch_size, num_active_dev=nd)
            return self.predict_device(preds, batch_size, anchors_mask=self.anchor_area_mask(vox["coordinates"], batch_size, nd))
        # SimpleVoxelRadius: rows [r, z, w, 0] from the voxeliser's epilogue, declared to the middle as pitch-4 rows
        enc, pitch = ({}, {}) if self.encoder == "SimpleVoxel" else ({"encoder": self.encoder}, {"in_pitch": SimpleVoxelRadius.ROW_PITCH})
        if not static:
            vox = self.voxel_generator.generate_device(points, point_offsets, mean_features=nf, mean_dtype=self._infer_dtype, **enc)
            preds = self.network_forward(vox["mean"], vox["coordinates"], batch_size, site_table=vox.get("site_table"), **pitch)
            nd = None
        else:
            # (the voxel means are stored in the sparse stack's dtype by the voxeliser itself: no cast launch inside the captured step)
            vox = self.voxel_generator.generate_device(points, point_offsets, mean_features=nf, sync=False, mean_dtype=self._infer_dtype, **enc)
            nd = vox["voxel_offsets"][batch_size:]
            preds = self.network_forward(vox["mean"], vox["coordinates"], batch_size,
                                         num_active_dev=nd, site_table=vox.get("site_table"), **pitch)
        return self.predict_device(preds, batch_size, anchors_mask=self.anchor_area_mask(vox["coordinates"], batch_size, nd))

    def anchor_area_mask(self, coors, batch_size, num_dev=None):
        """The config's anchor-area mask [B, A] uint8 from voxel coordinates [rows, 4] (b, z, y, x) -- what prep_pointcloud puts into the
        example as ``anchors_mask`` (preprocess.py:345-357) -- on the caller's stream (part of a captured forward_points); None when
        the config asks for none.  Kept as ``last_anchors_mask``."""
        thr = anchor_area_threshold_of(self.cfg)
        if thr is None:
            return None
        vs, rng = self.voxel_generator.voxel_size, self.voxel_generator.point_cloud_range       # float32, as the reference's generator keeps them
        gs = self.grid_size
        self.last_anchors_mask = ops.anchor_area_mask(coors, num_dev, batch_size, (int(gs[1]), int(gs[0])), self.anchors, vs[:2], rng[:2], thr)
        return self.last_anchors_mask

    def calibrate(self, points, point_offsets, margin=1.25):
        """Size the static-capacity buffers of the strided layers from one eager forward of representative
        clouds (live outputs x margin, rounded up to 256 rows), like a static-shape inference engine profile.
        Data that later exceeds a capacity is reported by :meth:`check_overflow`."""
        with torch.no_grad():
            self.forward_points(points, point_offsets)
        caps = []
        for m in self.middle_feature_extractor.modules():
            if isinstance(m, spconv.SparseConvolution) and not m.subm and m.last_num_out is not None:
                m.static_out_rows = int(-(-int(m.last_num_out * margin) // 256) * 256)
                caps.append(m.static_out_rows)
        return caps

    def check_overflow(self):
        """Raise if a strided layer of the last static forward (every branch of a branched graph) produced more
        outputs than its capacity."""
        checks = list(getattr(self.middle_feature_extractor, "last_overflow_checks", []))
        for lst in getattr(self, "_branch_overflow", []):
            checks += list(lst)
        for num, cap in checks:
            raw = int(num[1].item())
            if raw > cap:
                raise RuntimeError(f"static-capacity overflow: a strided sparse conv produced {raw} outputs, capacity {cap}")

    def make_graphed(self, points, point_offsets, warmup=3, branches=1, parts=None):
        """Capture the static forward into a hipGraph.  Returns (replay_fn, outputs); new clouds are fed by
        copying into ``points`` / ``point_offsets`` (any point count <= capacity) before calling replay_fn.

        ``branches`` > 1: the frames are split into that many contiguous groups, each captured as an independent
        branch of the SAME graph on its own stream (frames are independent).  Most kernels of the path are
        latency bound, so two half-batch chains overlap better than one full-batch chain (1.43 -> 1.33 ms for 8
        frames; 4 branches no better, 8 worse).  Returns (replay_fn, [outputs per branch], [(points_i, offsets_i)]):
        the per-branch input buffers are the ones to refill."""
        if branches <= 1:
            return self._capture([(points, point_offsets)], warmup)[:2]
        if parts is None:      # (``parts``: input buffers of an earlier capture, re-used so that several graphs read the same ones)
            offs = point_offsets.cpu().tolist()
            nfr = len(offs) - 1
            branches = min(branches, nfr)
            bounds = [round(i * nfr / branches) for i in range(branches + 1)]
            parts = []
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                pts = points[offs[lo]:offs[hi]].clone()
                po = torch.tensor([o - offs[lo] for o in offs[lo:hi + 1]], dtype=torch.int32, device=points.device)
                parts.append((pts, po))
        # capacities: the largest any branch needs
        caps = None
        for pts, po in parts:
            c = self.calibrate(pts, po)
            caps = c if caps is None else [max(a, b) for a, b in zip(caps, c)]
        if caps:
            mods = [m for m in self.middle_feature_extractor.modules()
                    if isinstance(m, spconv.SparseConvolution) and not m.subm and m.last_num_out is not None]
            for m, c in zip(mods, caps):
                m.static_out_rows = c
        replay, outs, _ = self._capture(parts, warmup)
        return replay, outs, parts

    def _capture(self, parts, warmup):
        mfe = self.middle_feature_extractor
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(warmup):
                for pts, po in parts:
                    self.forward_points(pts, po, static=True)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        outs, self._branch_overflow = [], []
        # thread_local: a RCCL watchdog / other host thread touching the runtime must not invalidate the capture
        with ops.rt.capture_guard(), torch.no_grad(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
            cur = torch.cuda.current_stream()
            side = [torch.cuda.Stream() for _ in parts[1:]]
            for st in side:
                st.wait_stream(cur)
            for st, (pts, po) in zip([cur] + side, parts):
                with torch.cuda.stream(st):
                    outs.append(self.forward_points(pts, po, static=True))
                    self._branch_overflow.append(list(getattr(self.middle_feature_extractor, "last_overflow_checks", [])))
            for st in side:
                cur.wait_stream(st)
        return graph.replay, (outs[0] if len(parts) == 1 else outs), graph

    def _capture_stages(self, points, point_offsets, warmup=3):
        """The static forward as THREE hipGraphs sharing one memory pool -- (A) voxelise + sparse middle, (B) the dense RPN, (C)
        decode / top-k / NMS -- so that a serving loop with several steps in flight can pass a token between the lanes' (B)
        segments (InFlightRunner(serialize_rpn=True)): the MFMA-bound RPN segments then run one after another while the
        latency-bound (A) / (C) segments of the other lanes run beside them.  Returns ((replay_a, replay_b, replay_c), outputs)."""
        assert not self.pillars and self._infer_dtype is not None, "staged capture: the sparse-middle inference path"
        batch_size = point_offsets.numel() - 1
        nf = self.cfg["num_point_features"]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(warmup):
                self.forward_points(points, point_offsets, static=True)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        pool = torch.cuda.graph_pool_handle()
        ga, gb, gc = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        prev = ops.set_rulebook_numbering(self.rulebook_numbering)
        try:
            with torch.no_grad():
                with ops.rt.capture_guard(), torch.cuda.graph(ga, pool=pool, capture_error_mode="thread_local"):
                    vox = self.voxel_generator.generate_device(points, point_offsets, mean_features=nf, sync=False,
                                                               mean_dtype=self._infer_dtype,
                                                               **({} if self.encoder == "SimpleVoxel" else {"encoder": self.encoder}))
                    pitch = {} if self.encoder == "SimpleVoxel" else {"in_pitch": SimpleVoxelRadius.ROW_PITCH}
                    spatial = self.middle_feature_extractor(vox["mean"].to(self._infer_dtype), vox["coordinates"], batch_size,
                                                            channels_last=True, num_active_dev=vox["voxel_offsets"][batch_size:],
                                                            site_table=vox.get("site_table"),
                                                            bev_sparse=self._rpn_takes_rows(), **pitch)
                    self._branch_overflow = [list(getattr(self.middle_feature_extractor, "last_overflow_checks", []))]
                    if isinstance(spatial, SparseBEV) and getattr(self.rpn, "background_convs", 0) and self.rpn.skip_background:
                        with self.lazy_heads(cover=True):
                            layers_, masks_, cover_ = self.rpn.tile_list_request(*spatial.spatial_shape[-2:])
                            spatial.tile_lists(layers_, masks=masks_, cover=cover_)   # the live-tile lists belong to the latency-bound segment
                with ops.rt.capture_guard(), torch.cuda.graph(gb, pool=pool, capture_error_mode="thread_local"):
                    with self.lazy_heads(cover=True):
                        preds = self.rpn(spatial)
                with ops.rt.capture_guard(), torch.cuda.graph(gc, pool=pool, capture_error_mode="thread_local"):
                    out = self.predict_device(preds, batch_size)
        finally:
            ops.set_rulebook_numbering(prev)
        # buffers the later graphs read: owned by whoever keeps the replays (InFlightRunner stores them per lane); the detector
        # only remembers the LAST capture, so rebuilding runners does not accumulate graph-pool buffers here
        self._last_stage_buffers = (vox, spatial, preds)
        return (ga.replay, gb.replay, gc.replay), out

    # -- post-processing -----------------------------------------------------------------------------
    def _select(self, preds, batch_size, anchors, anchors_mask=None):
        """score filter + top-k + decode of the selected boxes, all on device, fixed shapes.  ``anchors_mask`` [B, A]: anchors with a zero
        entry are dropped before the score threshold (voxelnet.py:429-439)."""
        cfg = self.cfg
        nc = cfg["num_class"]
        nd = self.box_ndim
        box = preds["box_preds"].reshape(batch_size, -1, nd)
        if nc == 1:
            scores = torch.sigmoid(preds["cls_preds"].reshape(batch_size, -1).float())
            labels = None
        else:   # class-agnostic selection: best class per anchor (voxelnet.py:545-553)
            scores, labels = torch.sigmoid(preds["cls_preds"].reshape(batch_size, -1, nc).float()).max(-1)
        k = min(cfg["nms_pre_max_size"], scores.shape[1])
        passing = scores >= cfg["nms_score_threshold"]
        if anchors_mask is not None:
            passing = passing & (anchors_mask.reshape(batch_size, -1) != 0)
        masked = torch.where(passing, scores, torch.full_like(scores, -1.0))
        top_scores, top_idx = torch.topk(masked, k, dim=1)
        counts = (top_scores >= cfg["nms_score_threshold"]).sum(1).to(torch.int32)
        enc = torch.gather(box, 1, top_idx.unsqueeze(-1).expand(-1, -1, nd)).float()
        anc = anchors[top_idx] if anchors.dim() == 2 else torch.gather(anchors, 1, top_idx.unsqueeze(-1).expand(-1, -1, nd))
        dec = decode_boxes(enc, anc)
        if "dir_cls_preds" in preds:
            d = preds["dir_cls_preds"].reshape(batch_size, -1, cfg["num_direction_bins"])
            d = torch.gather(d, 1, top_idx.unsqueeze(-1).expand(-1, -1, cfg["num_direction_bins"]))
            dir_labels = torch.max(d, dim=-1)[1]
        else:
            dir_labels = None
        top_labels = torch.gather(labels, 1, top_idx) if labels is not None else torch.zeros_like(top_idx)
        return dec, top_scores, counts, dir_labels, top_labels

    def _nms_kind(self):
        """(kind, semantics) of ops.nms_sorted for this config: nms.py's rotated NMS, or spconv's axis-aligned one on the standup boxes."""
        return ("rotate", "cpu") if self.cfg["use_rotate_nms"] else ("axis_aligned", "numba")

    def _nms_rows(self, dec, top_scores):
        """The NMS input rows of decoded boxes ``dec`` [B, k, 7] and their scores [B, k], plus :meth:`_nms_kind`."""
        if self.cfg["use_rotate_nms"]:
            # (x, y, w, l, r, score): boxes_for_nms = box[:, [0, 1, 3, 4, 6]] (voxelnet.py:570); slices, not index
            # lists, so that nothing is staged from the host (hipGraph capture)
            dets = torch.cat([dec[..., 0:2], dec[..., 3:5], dec[..., 6:7], top_scores.unsqueeze(-1)], -1).contiguous()
        else:
            # standup boxes of the rotated BEV rectangles (voxelnet.py:571-576 -> center_to_corner_box2d +
            # corner_to_standup_nd), then nms -> nms_gpu_cc -> spconv non_max_suppression ('+1', IoU > thr)
            hx, hy, ang = dec[..., 3] * 0.5, dec[..., 4] * 0.5, dec[..., 6]
            cs, sn = torch.cos(ang).abs(), torch.sin(ang).abs()
            ex, ey = hx * cs + hy * sn, hx * sn + hy * cs
            dets = torch.stack([dec[..., 0] - ex, dec[..., 1] - ey, dec[..., 0] + ex, dec[..., 1] + ey, top_scores], -1).contiguous()
        return (dets, *self._nms_kind())

    def _fix_direction_and_range(self, boxes, valid, dir_labels):
        """The direction fix of ``boxes`` [B, P, 7] in place (voxelnet.py:598-607; ``dir_labels`` [B, P], a list of per-class [B, P_c]
        to concatenate, or None) -> ``valid`` and the post_center_range mask (:611-621)."""
        cfg = self.cfg
        if dir_labels is not None:
            period = 2 * math.pi / cfg["num_direction_bins"]
            rot = limit_period(boxes[..., 6] - cfg["direction_offset"], cfg["direction_limit_offset"], period)
            boxes[..., 6] = rot + cfg["direction_offset"] + period * (torch.cat(dir_labels, 1) if isinstance(dir_labels, list)
                                                                      else dir_labels).to(boxes.dtype)
        r = self.post_center_range
        return valid & (boxes[..., :3] >= r[:3]).all(-1) & (boxes[..., :3] <= r[3:]).all(-1)

    def predict_device(self, preds, batch_size, anchors=None, anchors_mask=None):
        """-> dict of padded device tensors: boxes [B,P,box_ndim], scores [B,P], labels [B,P], valid [B,P] (bool).
        ``anchors_mask`` [B, A] bool / uint8 (the example's, or :meth:`anchor_area_mask`): frame b keeps the anchors with a non-zero entry."""
        cfg = self.cfg
        anchors = self.anchors if anchors is None else anchors
        several = isinstance(preds["cls_preds"], (list, tuple))      # a multi-head network's per-head views (MultiHeadInference)
        on_gpu = (preds["cls_preds"][0] if several else preds["cls_preds"]).is_cuda
        if self.multiclass is not None:
            if several:
                raise ValueError("multiclass_nms on a multi-head network (a list of head views) is not supported")
            if anchors_mask is not None:
                raise ValueError("multiclass_nms with anchors_mask is not supported (the reference indexes the masked arrays with "
                                 "unmasked anchor ranges there)")
            if on_gpu and self.fused_predict and max(self.multiclass["pre"]) <= 1024:
                return self._predict_multiclass_fused(preds, batch_size, anchors)
            return self._predict_multiclass(flat_preds(preds, batch_size), batch_size, anchors)
        if (on_gpu and self.fused_predict and cfg["nms_pre_max_size"] <= 1024 and (several or not self.heads) and not (several and anchors_mask is not None)):
            # (sec_predict_select ranks up to 1024 candidates per frame; larger nms_pre_max_size takes the torch.topk path
            # below, which honours it -- never a silent truncation.  A multi-head network's CONCATENATED predictions -- its module
            # graph's -- have no single [B, A, H, W, C] view: torch path too)
            return self._predict_fused(preds, batch_size, anchors, anchors_mask)
        preds = flat_preds(preds, batch_size)
        dec, top_scores, counts, dir_labels, top_labels = self._select(preds, batch_size, anchors, anchors_mask)
        dets, kind, sem = self._nms_rows(dec, top_scores)
        keep, num_keep = ops.nms_sorted(dets, counts, cfg["nms_iou_threshold"], kind, sem, post_max=cfg["nms_post_max_size"])
        p = min(cfg["nms_post_max_size"], keep.shape[1])
        valid = self._arange_p[:p].unsqueeze(0) < num_keep.unsqueeze(1)
        sel = torch.where(valid, keep[:, :p], torch.zeros_like(keep[:, :p])).long()   # slots past num_keep are undefined
        boxes = torch.gather(dec, 1, sel.unsqueeze(-1).expand(-1, -1, dec.shape[-1]))
        scores = torch.gather(top_scores, 1, sel)
        valid = self._fix_direction_and_range(boxes, valid, None if dir_labels is None else torch.gather(dir_labels, 1, sel))
        return {"boxes": boxes, "scores": scores, "labels": torch.gather(top_labels, 1, sel), "valid": valid}

    def _predict_multiclass(self, preds, batch_size, anchors):
        """use_multi_class_nms (voxelnet.py:458-547) in plain torch, fixed shapes: per class c its anchor range (all anchors when
        class-agnostic), sigmoid of column c, threshold, top pre_c, NMS with iou_c, at most post_c survivors in NMS order; classes
        concatenated in class order (label c), then the direction fix and the range mask.  What runs for CPU tensors and for a pre_c
        above 1024; P = sum of post_c.  A frame on which no class keeps anything has no valid row (the reference raises there)."""
        cfg, mc = self.cfg, self.multiclass
        nc = cfg["num_class"]
        cls = preds["cls_preds"].reshape(batch_size, -1, nc)
        box = preds["box_preds"].reshape(batch_size, -1, 7)
        hw = self.feature_map_size[1] * self.feature_map_size[2]
        dirs = preds["dir_cls_preds"].reshape(batch_size, -1, cfg["num_direction_bins"]) if "dir_cls_preds" in preds else None
        out_boxes, out_scores, out_labels, out_valid, out_dl = [], [], [], [], []
        for c in range(nc):
            lo, hi = mc["a_ranges"][c][0] * hw, mc["a_ranges"][c][1] * hw
            scores = torch.sigmoid(cls[:, lo:hi, c].float())
            k = min(mc["pre"][c], hi - lo)
            masked = torch.where(scores >= mc["thr"][c], scores, torch.full_like(scores, -1.0))
            top_scores, top_idx = torch.topk(masked, k, dim=1)
            counts = (top_scores >= mc["thr"][c]).sum(1).to(torch.int32)
            top_idx = top_idx + lo
            enc = torch.gather(box, 1, top_idx.unsqueeze(-1).expand(-1, -1, 7)).float()
            anc = anchors[top_idx] if anchors.dim() == 2 else torch.gather(anchors, 1, top_idx.unsqueeze(-1).expand(-1, -1, 7))
            dec = decode_boxes(enc, anc)
            dets, kind, sem = self._nms_rows(dec, top_scores)
            keep, num_keep = ops.nms_sorted(dets, counts, mc["iou"][c], kind, sem, post_max=mc["post"][c])
            p = mc["post"][c]
            keep = keep.to(top_idx.device)[:, :p]
            keep = torch.nn.functional.pad(keep, (0, p - keep.shape[1]))              # post_c slots even where fewer were selected
            valid = torch.arange(p, dtype=torch.int32, device=keep.device).unsqueeze(0) < num_keep.to(keep.device).unsqueeze(1)
            sel = torch.where(valid, keep, torch.zeros_like(keep)).long()
            out_boxes.append(torch.gather(dec, 1, sel.unsqueeze(-1).expand(-1, -1, 7)))
            out_scores.append(torch.gather(top_scores, 1, sel))
            out_labels.append(torch.full_like(sel, c))
            out_valid.append(valid)
            if dirs is not None:
                d = torch.gather(dirs, 1, top_idx.unsqueeze(-1).expand(-1, -1, cfg["num_direction_bins"]))
                out_dl.append(torch.gather(torch.max(d, dim=-1)[1], 1, sel))
        boxes, scores, valid = torch.cat(out_boxes, 1), torch.cat(out_scores, 1), torch.cat(out_valid, 1)
        valid = self._fix_direction_and_range(boxes, valid, None if dirs is None else out_dl)
        return {"boxes": boxes, "scores": scores, "labels": torch.cat(out_labels, 1), "valid": valid}

    def _head_views(self, preds, batch_size, anchors=None):
        """(cls, box, dir or None) of ``preds`` as [B, A, H, W, C] views -- a multi-head network's LISTS of such views (every view has
        its own [A_s, H_s, W_s]: the *_segments kernels) pass through -- and ``anchors`` as the flat float32 [N, 7] list the decode
        reads (None for heads that have none: the empty frame's maps behind lazy heads)."""
        cfg = self.cfg
        _, h, w = self.feature_map_size

        def view5(t, code):
            if isinstance(t, (list, tuple)):
                assert all(v.dim() == 5 for v in t)
                return list(t)
            return t if t.dim() == 5 else t.reshape(batch_size, self.num_anchor_per_loc, h, w, code)
        cls = view5(preds["cls_preds"], cfg["num_class"])
        box = view5(preds["box_preds"], self.box_ndim)
        dirp = view5(preds["dir_cls_preds"], cfg["num_direction_bins"]) if "dir_cls_preds" in preds else None
        if anchors is not None:
            anchors = (anchors[0] if anchors.dim() == 3 else anchors).float().contiguous()
        return cls, box, dirp, anchors

    def _predict_multiclass_fused(self, preds, batch_size, anchors):
        """:meth:`_predict_multiclass` on the device with (frame, class) items: select -> decode -> NMS (two launches) -> finalize from
        the head tensor in place, no host sync, no torch glue (capturable)."""
        cfg, mc = self.cfg, self.multiclass
        cls, box, dirp, anchors = self._head_views(preds, batch_size, anchors)
        dev = cls.device
        tab = mc["device"].get(dev)
        if tab is None:        # the per-class arrays the NMS and finalize kernels index (made once per device, outside any capture)
            tab = mc["device"][dev] = (torch.tensor(mc["iou"], dtype=torch.float32, device=dev),
                                       torch.tensor(mc["post"], dtype=torch.int32, device=dev),
                                       torch.tensor(mc["post_offsets"], dtype=torch.int32, device=dev))
        iou_t, post_t, off_t = tab
        top_idx, top_score, counts = ops.predict_select_classes(cls, mc["a_ranges"], mc["pre"], mc["thr"])
        dec, dets, dlab = ops.predict_decode_classes(box, dirp, anchors, top_idx, top_score, rotate=cfg["use_rotate_nms"])
        keep, num_keep = ops.nms_sorted_items(dets, counts, iou_t, post_t, *self._nms_kind())
        return ops.predict_finalize_classes(dec, top_score, dlab, keep, num_keep, off_t, mc["P"], dirp is not None,
                                            cfg["direction_offset"], cfg["direction_limit_offset"], cfg["num_direction_bins"],
                                            self.post_center_range)

    def _predict_fused(self, preds, batch_size, anchors, anchors_mask=None):
        """select -> decode -> NMS -> finalize: five launches, no host sync, no torch glue."""
        cfg = self.cfg
        cls, box, dirp, anchors = self._head_views(preds, batch_size, anchors)
        lz = preds.get("lazy_heads")       # (tile_live, empty-frame heads): background tiles of the head tensor were never written
        lz_cls = lz_box = None
        if lz is not None:
            bg_cls, bg_box, bg_dir, _ = self._head_views(lz[1], batch_size)
            lz_cls, lz_box = (lz[0], bg_cls), (lz[0], (bg_box, bg_dir if dirp is not None else None))
        top_idx, top_score, top_label, counts = ops.predict_select(cls, cfg["nms_pre_max_size"], cfg["nms_score_threshold"], lazy=lz_cls,
                                                                  anchor_mask=None if anchors_mask is None else anchors_mask.reshape(batch_size, -1))
        dec, dets, dlab = ops.predict_decode(box, dirp, anchors, top_idx, top_score, rotate=cfg["use_rotate_nms"], lazy=lz_box)
        kind, sem = self._nms_kind()
        keep, num_keep = ops.nms_sorted(dets, counts, cfg["nms_iou_threshold"], kind, sem, post_max=cfg["nms_post_max_size"])
        return ops.predict_finalize(dec, top_score, top_label, dlab, keep, num_keep, cfg["nms_post_max_size"],
                                    dirp is not None, cfg["direction_offset"], cfg["direction_limit_offset"],
                                    cfg["num_direction_bins"], self.post_center_range)

    def predict(self, preds, anchors, anchors_mask=None):
        out = self.predict_device(preds, anchors.shape[0], anchors, anchors_mask)
        res = []
        for b in range(anchors.shape[0]):
            m = out["valid"][b]
            res.append({"box3d_lidar": out["boxes"][b][m], "scores": out["scores"][b][m],
                        "label_preds": out["labels"][b][m], "metadata": None})
        return res


def lane_stream(device=None, index=None):
    """A stream for one lane of a serving loop.  HIP maps streams onto a handful of hardware queues (GPU_MAX_HW_QUEUES, default 4) per
    PRIORITY level, handing a new stream the least-shared queue: whether two lanes end up behind each other in one queue then depends
    on how many other streams the process created before (torch's capture / warm-up side streams included) -- measured on the same
    loop: 17.0 k, 13.3 k or 9.4 k frames/s depending on it.  High-priority streams come from a queue pool of their own that nothing
    else in the process uses, so a few lanes get a queue each whatever ran before.  SEC_LANE_PRIORITY=0: normal-priority streams."""
    import os
    groups = int(os.environ.get("SEC_LANE_CU_GROUPS", "0") or 0)
    if groups > 1 and index is not None:
        return _cu_masked_stream(index % groups, groups)
    prio = -1 if os.environ.get("SEC_LANE_PRIORITY", "-1") != "0" else 0
    return torch.cuda.Stream(device=device, priority=prio)


_masked_streams = []          # (hipStream_t, ExternalStream): kept alive for the life of the process


def _cu_masked_stream(group, groups):
    """EXPERIMENT (SEC_LANE_CU_GROUPS=g): a stream whose kernels run on the ``group``-th of ``groups`` equal slices of every XCD's CUs
    (hipExtStreamCreateWithCUMask; mask bit i = CU slot i // 8 of XCD i % 8 on MI355X, ``tools/probes/cu_mask_probe.hip``), so that lanes of
    different groups never share a CU and every chip-filling launch of a lane becomes several rounds on its own slice."""
    import ctypes
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    hip = ctypes.CDLL(path)
    slots = 32 // groups                                   # CU slots per XCD and group
    bits = 0
    for slot in range(group * slots, (group + 1) * slots):
        bits |= 0xff << (8 * slot)
    words = (ctypes.c_uint32 * 8)(*[(bits >> (32 * w)) & 0xffffffff for w in range(8)])
    st = ctypes.c_void_p()
    rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(st), 8, words)
    if rc != 0:
        raise RuntimeError(f"hipExtStreamCreateWithCUMask -> {rc}")
    ext = torch.cuda.ExternalStream(st.value)
    _masked_streams.append((st, ext))
    return ext


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class InFlightRunner:
    """Serving loop with several steps in flight: ``inflight`` captured forwards (hipGraphs with their own activation
    buffers, all reading the same resident input buffers -- ``points`` / ``point_offsets``, or ``self.parts`` with branches)
    are replayed round-robin on their own HIP streams.  Replays on
    one lane serialise, different lanes overlap -- the latency-bound sparse stages of one step run beside the MFMA-bound
    RPN of another (car.fhd, batch 8: 5600 -> 7200 frames/s with three lanes; more lanes add nothing).
    ``serialize_rpn``: a step is three graphs (sparse front / RPN / predict) and the lanes hand a token (an event) from RPN
    segment to RPN segment, so that at most ONE lane is in its MFMA-bound segment at any time: uncoordinated lanes now and then
    sit in their RPN segments together (the others' launches wait for conv tiles to retire) or all in their latency-bound
    segments (matrix pipes idle).  Round 3: 14.0 k -> 14.7 k frames/s with four lanes (three lanes: 14.4 k; five: 13.3 k; the RPN
    segments on one extra stream with or without a CU mask instead of the token: 11.5 k -- the event ping-pong costs more than it
    orders; `gpurun_out` r03_as-au).

    ``step()`` enqueues one full forward and returns (outputs, stream): the output tensors of that lane, valid once
    ``stream`` has been synchronised (or after :meth:`synchronize`) and until the lane is stepped again."""

    def __init__(self, det, points, point_offsets, inflight=3, branches=1, private_inputs=False, serialize_rpn=False, rpn_tokens=None):
        """``private_inputs``: every lane gets its OWN copy of the input buffers (``self.inputs[k]``) and pinned host
        mirrors of its outputs, so that :meth:`step` can take a host-resident batch: the pinned-host -> HBM copy of lane k's
        next clouds then overlaps the compute of the other lanes (the end-to-end serving form; with shared buffers a copy
        would race with the lanes still reading them)."""
        self.det = det
        self.replays, self.outputs, self.parts = [], [], None
        self.inputs, self.host_outputs = [], []
        self._overflow = []                       # overflow counters of EVERY lane (each capture has its own rulebook buffers)
        # ``serialize_rpn``: every lane's step is three graphs (SecondDetector._capture_stages) and the RPN segments pass a token
        # (an event) from lane to lane: at most one lane is in its MFMA-bound segment at a time, the others' latency-bound
        # segments fill the rest of the chip
        self.serialize_rpn = bool(serialize_rpn) and branches <= 1 and int(inflight) > 1
        self._rpn_token = None
        # RPN segments allowed at a time (a ring of that many events); None = decided after the captures from the scene (below)
        self.rpn_tokens = None if rpn_tokens is None else max(1, int(rpn_tokens))
        self._rpn_events = []
        self._keepalive = []                      # per lane: the buffers its three graphs hand to each other
        assert not (private_inputs and branches > 1), "private input buffers are a single-chain feature"
        for _ in range(max(1, int(inflight))):
            if self.serialize_rpn:
                pk, ok = (points.clone(), point_offsets.clone()) if private_inputs else (points, point_offsets)
                replay, outs = det._capture_stages(pk, ok)
                self._keepalive.append(det._last_stage_buffers)
                self.inputs.append((pk, ok))
                if private_inputs:
                    self.host_outputs.append({k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in outs.items()})
            elif branches > 1:
                # the per-branch input buffers are created by the first lane and shared by all others: one place to refill
                replay, outs, self.parts = det.make_graphed(points, point_offsets, branches=branches, parts=self.parts)
            else:
                pk, ok = (points.clone(), point_offsets.clone()) if private_inputs else (points, point_offsets)
                replay, outs = det.make_graphed(pk, ok)
                self.inputs.append((pk, ok))
                if private_inputs:
                    self.host_outputs.append({k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in outs.items()})
            self.replays.append(replay)
            self.outputs.append(outs)
            self._overflow += [c for lst in getattr(det, "_branch_overflow", []) for c in lst]
        if self.rpn_tokens is None:
            # Two RPN segments at a time when the RPN is the light part of the step -- the calibration scene leaves most of the last conv's
            # tiles to the background -- and one when the scene is dense.  Measured with four lanes, interleaved runs (gpurun r06_lanes3 /
            # r06_tok2; round 6, since the last RPN conv carries the 1x1 tail): car.fhd (39 % of the tiles live) one token 20.2-20.3 k
            # frames/s, two 20.9 k, three 20.4-20.5 k, unserialised 20.5 k; dense seeded scene (81 % live) 8.45 k with one, 8.38 k with two.
            # (Before the tail moved, one and two tokens were level: 20.0 / 20.1 k, r05_j.)
            self.rpn_tokens = 1
            counts = getattr(det.rpn, "last_live_counts", None)
            if self.serialize_rpn and counts is not None and getattr(det.rpn, "skip_background", False):
                for seg in self.replays[-1]:          # the counts are the last capture's buffer: one replay of that lane fills it
                    seg()
                torch.cuda.synchronize()
                tiles = getattr(det.rpn, "last_tiles_per_frame", None)
                if tiles:
                    last = min(det.rpn.background_convs, counts.shape[0]) - 1
                    share = float(counts[last].sum().item()) / float(tiles * counts.shape[1])
                    self.rpn_tokens = 2 if share <= 0.6 else 1
        self.lanes = [lane_stream(index=i) for i in range(len(self.replays))] if len(self.replays) > 1 else [None]
        self._k = 0

    def step(self, host_points=None, host_offsets=None, fetch=False):
        """Enqueue one full forward on the next lane.  ``host_points`` [n <= capacity, F] / ``host_offsets`` [B + 1] (pinned
        host tensors; needs ``private_inputs``): copied into the lane's input buffers on the lane's stream ahead of the
        replay.  ``fetch``: the lane's detections are copied to its pinned host mirrors (``self.host_outputs[k]``) behind the
        replay.  Nothing here synchronises the host."""
        k = self._k % len(self.replays)
        self._k += 1
        lane = self.lanes[k]
        ctx = torch.cuda.stream(lane) if lane is not None else _NullCtx()
        with ctx:
            if host_points is not None:
                pk, ok = self.inputs[k]
                pk[:host_points.shape[0]].copy_(host_points, non_blocking=True)
                ok.copy_(host_offsets, non_blocking=True)
            if self.serialize_rpn:
                ra, rb, rc = self.replays[k]
                st = lane if lane is not None else torch.cuda.current_stream()
                ra()
                if len(self._rpn_events) >= self.rpn_tokens:
                    st.wait_event(self._rpn_events[-self.rpn_tokens])   # the RPN segment `rpn_tokens` steps back (another lane) has finished
                rb()
                ev = torch.cuda.Event()
                ev.record(st)
                self._rpn_events = (self._rpn_events + [ev])[-self.rpn_tokens:]
                rc()
            else:
                self.replays[k]()
            if fetch:
                for name, t in self.outputs[k].items():
                    self.host_outputs[k][name].copy_(t, non_blocking=True)
        return self.outputs[k], (lane if lane is not None else torch.cuda.current_stream())

    def synchronize(self):
        torch.cuda.synchronize()
        for num, cap in self._overflow:
            raw = int(num[1].item())
            if raw > cap:
                raise RuntimeError(f"static-capacity overflow: a strided sparse conv produced {raw} outputs, capacity {cap}")


def decode_boxes(enc, anc):
    """GroundBox3dCoder.decode (second_box_decode, second/pytorch/core/box_torch_ops.py:56-101); columns 7.. (custom values): t + a."""
    xa, ya, za, wa, la, ha, ra = anc[..., :7].unbind(-1)
    xt, yt, zt, wt, lt, ht, rt = enc[..., :7].unbind(-1)
    diag = torch.sqrt(la * la + wa * wa)
    return torch.stack([xt * diag + xa, yt * diag + ya, zt * ha + za, torch.exp(wt) * wa, torch.exp(lt) * la,
                        torch.exp(ht) * ha, rt + ra, *(enc[..., 7:] + anc[..., 7:]).unbind(-1)], -1)
