"""Host side of training the multi-head network (no GPU): argument validation of sec_pfn_radius_train_fwd / _bwd before anything is
enqueued, the two trainers' refusals, the reduced-geometry config of the GPU trainer tests, and models.multihead_forward_mixed in
float32 on the CPU against the module graph."""
import ctypes

import numpy as np
import pytest
import torch

from mhead_train_helpers import small_cfg


def test_radius_training_entry_points_validate_before_any_launch():
    """Status codes of include/second_hip.h, decided on the host exactly as sec_pfn_train_fwd / _bwd decide them."""
    from second_amd import runtime as rt
    l = rt.lib()
    one = ctypes.c_void_p(4096)                       # a non-NULL pointer that is never dereferenced on these paths
    big = 1 << 30

    def fwd(t=60, f=4, c=64, out=one, arg=one, stats=one, ws=one, wsb=big, p=100):
        return l.sec_pfn_radius_train_fwd(one, one, one, p, t, f, one, one, one, 1e-3, 0.01, one, one, c, 0.25, 0.25, 0.0, 0.0, out, arg,
                                          stats, ws, wsb, None)

    def bwd(t=60, f=4, c=64, stats=one, arg=one, dw=one, dg=one, db=one, ws=one, wsb=big, p=100):
        return l.sec_pfn_radius_train_bwd(one, one, one, p, t, f, one, one, stats, c, 0.25, 0.25, 0.0, 0.0, one, one, arg, dw, dg, db,
                                          ws, wsb, None)
    assert fwd(stats=None) == -1 and fwd(arg=None) == -1 and fwd(out=None) == -1
    assert bwd(stats=None) == -1 and bwd(arg=None) == -1 and bwd(dw=None) == -1 and bwd(dg=None) == -1 and bwd(db=None) == -1
    assert fwd(t=128) == -1 and bwd(t=128) == -1                    # the int8 argmax holds slots 0..126 and -1
    assert fwd(f=5) == -3 and bwd(f=5) == -3 and fwd(c=65) == -3 and bwd(c=65) == -3
    need = l.sec_pfn_train_workspace_bytes(100, 64)
    assert need > 0
    assert fwd(wsb=need - 1) == -2 and bwd(wsb=need - 1) == -2 and fwd(ws=None) == -2 and bwd(ws=None) == -2
    # the checks come before the empty-input return as well
    assert fwd(p=0, t=128) == -1 and fwd(p=0, c=65) == -3 and fwd(p=-1) == -1 and bwd(p=-1) == -1
    assert fwd(p=0) == 0                                              # a no-op: nothing is launched, no device is touched


def test_trainers_refuse_the_other_kind_of_network_by_name():
    from second_amd import models as M, training
    with pytest.raises(NotImplementedError, match="MultiHeadDeviceTrainer"):
        training.DeviceTrainer(M.SecondDetector(small_cfg()))
    with pytest.raises(NotImplementedError, match="multi-head network .*MultiHeadDeviceTrainer"):
        training.DeviceTrainer(M.SecondDetector(M.ALL_PP_MHEAD))
    with pytest.raises(NotImplementedError, match=f"MultiHeadDeviceTrainer: {M.ALL_PP_LARGEA['name']} is a single-head network"):
        training.MultiHeadDeviceTrainer(M.SecondDetector(M.ALL_PP_LARGEA))
    assert issubclass(training.MultiHeadDeviceTrainer, training.DeviceTrainer)


def test_reduced_geometry_config_builds_with_the_recorded_anchors(golden):
    from second_amd import models as M
    cfg = small_cfg()
    det = M.SecondDetector(cfg)
    assert det.feature_map_size == [1, 20, 20] and det.pillars and isinstance(det.voxel_feature_extractor, M.PillarFeatureNetRadius)
    assert tuple(det.anchors.shape) == (4800 + 8192, 7)
    np.testing.assert_array_equal(det.anchors.numpy(), golden("mhead")["anchors_small_geometry"])
    assert M.anchor_class_ranges(cfg, det.feature_map_size)[-1] == 12992
    names = {n.split(".")[0] for n, _ in det.named_parameters()}
    assert {"small_head", "large_head", "rpn", "voxel_feature_extractor"} <= names


def test_multihead_forward_mixed_in_float32_is_the_module_graph():
    """The same modules in the same order on the CPU: only BatchNorm's batch reductions may differ (torch.allclose defaults).  The
    running statistics move alike: trunk norms with momentum 0.01, the tower's with 0.1."""
    import copy
    from second_amd import models as M
    torch.manual_seed(3)
    det = M.SecondDetector(small_cfg()).train()
    twin = copy.deepcopy(det)
    x = torch.randn(2, 64, 80, 80) * (torch.rand(2, 1, 80, 80) < 0.3)
    out = det.rpn(x)
    c = M.stage0_crop(out["stage0"].shape[2])
    small, large = det.small_head(out["stage0"][:, :, c:-c, c:-c]), det.large_head(out["out"])
    want = {k: torch.cat([large[k], small[k]], dim=1) for k in large}
    got = M.multihead_forward_mixed(twin, x, torch.float32)
    assert set(got) == {"box_preds", "cls_preds", "dir_cls_preds"}
    for k in want:
        assert got[k].shape == want[k].shape == (2, 12992, {"box_preds": 7, "cls_preds": 10, "dir_cls_preds": 2}[k])
        assert torch.allclose(got[k], want[k]), k
    sd, sd2 = det.state_dict(), twin.state_dict()
    moved = 0
    for k in sd:
        if "running_" in k or "num_batches" in k:
            assert torch.allclose(sd[k].float(), sd2[k].float()), k
            moved += int(k.endswith("num_batches_tracked") and int(sd[k]) == 1)
    assert moved == 3 + 4 + 6 + 6 + 3              # tower, block 0..2 and the three deblocks; the PFN norm did not run
    # gradients reach both heads and the tower through the function
    sum(v.float().square().mean() for v in got.values()).backward()
    for name in ("small_head.net.0.weight", "small_head.conv_cls.weight", "large_head.conv_box.bias", "rpn.blocks.0.1.weight"):
        g = dict(twin.named_parameters())[name].grad
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, name
