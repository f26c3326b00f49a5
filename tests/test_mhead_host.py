"""Host side of the multi-head network (no GPU): per-class anchor maps against the reference's target assigner (fixture recorded by
tests/golden/make_golden_mhead.py), argument validation of the *_segments entry points before anything is enqueued, the crop rule
and the class-order check."""
import ctypes

import numpy as np
import pytest
import torch


def _small_geometry(cfg):
    lim = lambda r: [(-8.0 if v == -40 else 8.0 if v == 40 else -10.0 if v == -50 else 10.0 if v == 50 else v) for v in r]
    return dict(cfg, point_cloud_range=[-10, -10, -5, 10, 10, 3], anchor_ranges=[lim(r) for r in cfg["anchor_ranges"]],
                group_feature_map_sizes=[[1, 20, 20]] * 5 + [[1, 32, 32]] * 5)


def test_generate_anchors_honours_per_class_feature_maps(golden):
    from second_amd import models as M
    g = golden("mhead")
    cfg = _small_geometry(M.ALL_PP_MHEAD)
    a = M.generate_anchors(cfg, [1, 20, 20])
    assert a.shape == (4800 + 8192, 7) == g["anchors_small_geometry"].shape and a.dtype == np.float32
    np.testing.assert_array_equal(a, g["anchors_small_geometry"])
    assert M.anchor_class_ranges(cfg, [1, 20, 20]) == [0, 800, 1600, 2400, 4000, 4800, 6848, 8896, 10944, 11968, 12992]
    # the config's own geometry
    full = M.anchor_class_ranges(M.ALL_PP_MHEAD, [1, 100, 100])
    assert full[5] == 120000 and full[-1] == 324800 and M.anchors_per_location(M.ALL_PP_MHEAD) == 20
    # configs without per-class maps are what they were
    assert M.anchor_class_ranges(M.ALL_PP_LARGEA, [1, 50, 50])[-1] == 12 * 2500
    assert list(g["anchor_classes"]) == ["bus", "car", "construction_vehicle", "trailer", "truck", "barrier", "bicycle", "motorcycle",
                                         "pedestrian", "traffic_cone"]


def test_config_values_and_refusals():
    from second_amd import models as M
    c = M.ALL_PP_MHEAD
    assert c["point_cloud_range"] == [-50, -50, -5, 50, 50, 3] and c["voxel_size"] == [0.25, 0.25, 8] and c["max_points_per_voxel"] == 60
    assert (c["nms_pre_max_size"], c["nms_post_max_size"], c["nms_score_threshold"], c["nms_iou_threshold"]) == (1000, 300, 0.05, 0.5)
    assert c["use_rotate_nms"] is False and c["direction_offset"] == 0.78 and c["group_rotations"] == {8: [0], 9: [0]}
    assert [h["num_anchor_per_loc"] for h in c["heads"]] == [12, 8]
    assert M.stage0_crop(200) == 20 and M.stage0_crop(36) == 4 and M.stage0_crop(25) == 2        # numpy rounding: half to even
    with pytest.raises(ValueError, match="crop"):
        M.stage0_crop(4)
    # a class of the stage0 map ahead of a class of the out map: refused by name
    swapped = dict(c, group_feature_map_sizes=[[1, 160, 160]] + [[1, 100, 100]] * 4 + [[1, 160, 160]] * 4 + [[1, 100, 100]])
    with pytest.raises(ValueError, match="class order"):
        M.SecondDetector(swapped)
    det = M.SecondDetector(dict(_small_geometry(c), heads=[dict(c["heads"][0], feature_map_size=[1, 20, 20]),
                                                           dict(c["heads"][1], feature_map_size=[1, 32, 32])]))
    keys = set(det.state_dict())
    assert {"small_head.net.0.weight", "small_head.net.7.running_var", "small_head.conv_cls.weight", "large_head.conv_dir_cls.bias",
            "voxel_feature_extractor.pfn_layers.0.linear.weight", "rpn.deblocks.2.0.weight"} <= keys
    assert not any(k.startswith("rpn.conv_") for k in keys)
    assert tuple(det.voxel_feature_extractor.pfn_layers[0].linear.weight.shape) == (64, 8)
    assert det.small_head.net[1].eps == 1e-5 and det.rpn.blocks[0][2].eps == 1e-3
    assert tuple(det.small_head.conv_cls.weight.shape) == (80, 64, 1, 1) and tuple(det.large_head.conv_box.weight.shape) == (84, 384, 1, 1)
    from second_amd import training
    with pytest.raises(NotImplementedError, match="multi-head"):
        training.DeviceTrainer(det)


def test_torch_formulation_of_the_radius_pfn_matches_the_reference_module(golden):
    """CPU: the module's torch formulation (grad mode, CPU) on the recorded pillars."""
    from second_amd import models as M
    g = golden("mhead")
    vfe = M.PillarFeatureNetRadius(4, [64], [0.25, 0.25, 8], [-50, -50, -5, 50, 50, 3]).eval()
    sd = {k[len("pfn_sd."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("pfn_sd.")}
    missing = vfe.load_state_dict(sd, strict=False)
    assert missing.missing_keys == ["pfn_layers.0.norm.num_batches_tracked"] or not missing.missing_keys
    with torch.no_grad():
        out = vfe(torch.from_numpy(g["pfn_voxels"]), torch.from_numpy(g["pfn_num_points"]), torch.from_numpy(g["pfn_coords"]))
    np.testing.assert_allclose(out.numpy(), g["pfn_out"], rtol=1e-4, atol=1e-5)
    assert M.VFES["PillarFeatureNetRadius"] is M.PillarFeatureNetRadius


def test_segment_entry_points_validate_before_any_launch():
    """Return codes of include/second_hip.h, decided on the host: SEC_E_INVALID (-1) for a segment count outside 1..4 or a NULL
    segment, SEC_E_UNSUPPORTED (-3) for k > 1024."""
    from second_amd import runtime as rt
    l = rt.lib()
    one = ctypes.c_void_p(4096)                       # never dereferenced: validation fails first
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
    strides = (ctypes.c_int64 * 20)(*([1] * 20))
    dims = (ctypes.c_int * 12)(*([2, 3, 4] * 4))
    sel = lambda s, p, k, keys=one, d=dims: l.sec_predict_select_segments(s, p, strides, d, 1, 1, k, 0.3, keys, one, one, one, one, rt.SEC_F32, None)
    assert sel(0, ptrs(4096), 10) == -1 and sel(5, ptrs(*[4096] * 5), 10) == -1 and sel(-1, ptrs(4096), 10) == -1
    assert sel(2, ptrs(4096, None), 10) == -1 and sel(1, ptrs(None), 10) == -1 and sel(1, None, 10) == -1
    assert sel(1, ptrs(4096), 1025) == -3 and sel(4, ptrs(*[4096] * 4), 2000) == -3
    assert sel(1, ptrs(4096), 0) == -1
    assert sel(1, ptrs(4096), 10, keys=None) == -2                                  # no key scratch
    assert sel(1, ptrs(4096), 10, d=(ctypes.c_int * 3)(2, 0, 4)) == -1              # an empty map
    dec = lambda s, p, d, k: l.sec_predict_decode_segments(s, p, strides, d, strides, dims, 2, 1, k, one, one, one, 0, one, one, one, rt.SEC_F32, None)
    assert dec(0, ptrs(4096), None, 10) == -1 and dec(5, ptrs(*[4096] * 5), None, 10) == -1
    assert dec(2, ptrs(4096, None), None, 10) == -1 and dec(2, ptrs(4096, 4096), ptrs(4096, None), 10) == -1
    assert dec(1, ptrs(4096), None, 1025) == -3
    assert dec(1, ptrs(4096), None, 0) == -1
