"""Drop-in check for ``nuscenes/all.pp.mhead.config`` (build container only: needs the reference checkout): the UNMODIFIED reference
network (VoxelNetNuscenesMultiHead: PillarFeatureNetRadius + PointPillarsScatter + RPNNoHead + SmallObjectHead / DefaultHead) runs
over this repository's ``spconv`` package, and the SecondDetector mirror computes the same heads and detections from the same state
dict.  CPU, oracle backend -- in the manner of test_reference_pointpillars_over_our_stack.  Also pins tests/reference_standin_mhead.py
(what the GPU tests accelerate) to the real network."""
import os

import numpy as np
import pytest
import torch

REF = os.environ.get("SECOND_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def ref():
    if not os.path.isdir(os.path.join(REF, "second")):
        pytest.skip("reference checkout not present")
    from second_amd import compat
    compat.install(REF)
    import second.pytorch.train as train
    return train


def _model_cfg(pre_max=None):
    from google.protobuf import text_format
    from second.protos import pipeline_pb2
    cfg = pipeline_pb2.TrainEvalPipelineConfig()
    text_format.Merge(open(os.path.join(REF, "second/configs/nuscenes/all.pp.mhead.config")).read(), cfg)
    if pre_max:
        for cs in cfg.model.second.target_assigner.class_settings:
            cs.nms_pre_max_size = pre_max                          # keeps the pure-Python iou_jit fast
    return cfg.model.second


def _assert_cfg_equal(got, want, skip=("name",)):
    for k in (set(got) & set(want)) - set(skip):
        a, b = got[k], want[k]
        if isinstance(a, float) or (isinstance(a, list) and a and isinstance(a[0], float)):
            np.testing.assert_allclose(a, b, rtol=1e-6, err_msg=k)           # values the network keeps in float32
        else:
            assert a == b, (k, a, b)


@pytest.fixture(scope="module")
def built(ref):
    import oracle_backend
    train = ref
    torch.manual_seed(0)
    with oracle_backend.installed():
        net = train.build_network(_model_cfg(200)).eval()
    g = torch.Generator().manual_seed(1)
    for m in net.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.running_mean.copy_(torch.empty_like(m.running_mean).uniform_(-0.1, 0.1, generator=g))
            m.running_var.copy_(torch.empty_like(m.running_var).uniform_(0.5, 1.5, generator=g))
    return net


def test_reference_multi_head_pointpillars_over_our_stack(ref, built):
    import oracle_backend
    from second_amd import dropin, synthetic as syn
    from second_amd.models import ALL_PP_MHEAD, SecondDetector
    train, net = ref, built
    assert type(net).__name__ == "VoxelNetNuscenesMultiHead"
    want_cfg = dict(ALL_PP_MHEAD, nms_pre_max_size=200, max_voxels=int(net.voxel_generator._max_voxels))
    _assert_cfg_equal(dropin.model_config(net), want_cfg)
    with oracle_backend.installed():
        cloud = syn.syn_nusc_cloud(0, num_points=20000, point_cloud_range=(-50, -50, -5, 50, 50, 3))
        vox = net.voxel_generator.generate(cloud, 30000)
        anchors = net.target_assigner.generate_anchors([1, 100, 100])["anchors"].reshape(1, -1, 7)
        assert anchors.shape == (1, 324800, 7)
        example = {"voxels": vox["voxels"], "num_points": vox["num_points_per_voxel"],
                   "coordinates": np.pad(vox["coordinates"], ((0, 0), (1, 0)), mode="constant", constant_values=0),
                   "anchors": anchors}
        ex = train.example_convert_to_torch(example, torch.float32, torch.device("cpu"))
        with torch.no_grad():
            ref_preds = net.network_forward(ex["voxels"], ex["num_points"], ex["coordinates"], 1)
        det = SecondDetector(dict(ALL_PP_MHEAD, nms_pre_max_size=200)).eval()
        theirs = net.state_dict()
        missing = det.load_state_dict({k: v for k, v in theirs.items() if k in det.state_dict()})
        assert not missing.missing_keys
        parts = ("voxel_feature_extractor", "middle_feature_extractor", "rpn", "small_head", "large_head")
        for k, v in theirs.items():
            if k.split(".")[0] in parts:
                assert k in det.state_dict() and tuple(det.state_dict()[k].shape) == tuple(v.shape), k
        assert det.anchors.shape == (324800, 7)
        np.testing.assert_allclose(det.anchors.numpy(), anchors[0], rtol=0, atol=1e-5)
        with torch.no_grad():
            feats = det.voxel_feature_extractor(ex["voxels"], ex["num_points"], ex["coordinates"])
            ours_preds = det.network_forward(feats, ex["coordinates"], 1)
        for k in ("box_preds", "cls_preds", "dir_cls_preds"):
            assert ours_preds[k].shape == ref_preds[k].shape
            np.testing.assert_allclose(ours_preds[k].numpy(), ref_preds[k].numpy(), rtol=1e-3, atol=1e-4)
        gen = torch.Generator().manual_seed(3)
        fake = {k: v.clone() for k, v in ref_preds.items()}
        fake["cls_preds"] = torch.randn(fake["cls_preds"].shape, generator=gen) * 0.8 - 5.2
        fake["box_preds"] = torch.randn(fake["box_preds"].shape, generator=gen) * 0.2
        fake["dir_cls_preds"] = torch.randn(fake["dir_cls_preds"].shape, generator=gen)
        with torch.no_grad():
            r = net.predict(ex, {k: v.clone() for k, v in fake.items()})[0]
            o = det.predict(fake, ex["anchors"].view(1, -1, 7))[0]
    assert r["scores"].shape[0] > 5
    np.testing.assert_allclose(o["scores"].numpy(), r["scores"].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(o["box3d_lidar"].numpy(), r["box3d_lidar"].numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_array_equal(o["label_preds"].numpy(), r["label_preds"].numpy())


def test_mhead_standin_is_shaped_like_the_reference_network(ref, built):
    """tests/reference_standin_mhead.py against the real build_network result: same sub-module type names, same state-dict keys and
    shapes, the tower's default-eps norms, and dropin.model_config reads the SAME configuration from both objects."""
    import oracle_backend
    import reference_standin_mhead
    from second_amd import dropin, models
    real = built
    with oracle_backend.installed():
        fake = reference_standin_mhead.build_voxelnet_mhead(dict(models.ALL_PP_MHEAD, nms_pre_max_size=200,
                                                                 max_voxels=int(real.voxel_generator._max_voxels))).eval()
    parts = ("voxel_feature_extractor", "middle_feature_extractor", "rpn", "small_head", "large_head")
    for part in parts:
        assert type(getattr(real, part)).__name__ == type(getattr(fake, part)).__name__
    assert type(real).__name__ == type(fake).__name__ == "VoxelNetNuscenesMultiHead"
    keys = lambda sd: {k: tuple(v.shape) for k, v in sd.items() if k.split(".")[0] in parts}
    assert keys(real.state_dict()) == keys(fake.state_dict())
    for a, b in zip(real.small_head.net, fake.small_head.net):
        if isinstance(a, torch.nn.BatchNorm2d):
            assert a.eps == b.eps == 1e-5 and a.momentum == b.momentum
    assert sorted(real.small_classes) == sorted(fake.small_classes) and list(real.target_assigner.classes) == list(fake.target_assigner.classes)
    c_real, c_fake = dropin.model_config(real), dropin.model_config(fake)
    assert set(c_real) == set(c_fake)
    _assert_cfg_equal(c_fake, c_real)


def test_networks_outside_the_multi_head_path_are_refused_by_name(ref):
    import oracle_backend
    from second_amd import dropin
    train = ref
    mcfg = _model_cfg()
    order = list(mcfg.target_assigner.class_settings)
    # barrier (a class of the stage0 map) ahead of the out map's classes
    swapped = [order[5]] + order[:5] + order[6:]
    del mcfg.target_assigner.class_settings[:]
    mcfg.target_assigner.class_settings.extend(swapped)
    with oracle_backend.installed():
        net = train.build_network(mcfg).eval()
        with pytest.raises(dropin.NotAccelerable, match="class order"):
            dropin.model_config(net)
