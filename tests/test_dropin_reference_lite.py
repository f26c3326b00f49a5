"""Drop-in check for ``car.lite.config``, ``people.fhd.config`` and KITTI ``all.fhd.config`` (build container only: needs the reference checkout): the
network the reference's own ``build_network`` returns is adopted by ``compat.accelerate_model`` -- configuration read off the
object, parameters moved by state-dict key -- and ``net(example)`` returns what the original forward returns.  CPU, oracle
backend (dynamic-shape mode of the engine); the static-capacity / graph mode on the stand-ins is tests/test_gpu_lite.py, and the
stand-ins are pinned to the real networks here."""
import os

import numpy as np
import pytest
import torch

REF = os.environ.get("SECOND_REFERENCE", "/root/reference")

CASES = [
    ("car.lite.config", "CAR_LITE", [1, 160, 132],
     dict(vfe="SimpleVoxelRadius", middle="SpMiddleFHDLite", middle_in=3, downsample_factor=8, num_anchor_per_loc=2, num_class=1,
          max_points_per_voxel=1, use_rotate_nms=True, num_point_features=4)),
    ("people.fhd.config", "PEOPLE_FHD", [1, 200, 240],
     dict(middle="SpMiddleFHDPeople", middle_in=4, downsample_factor=4, num_anchor_per_loc=4, num_class=2,
          max_points_per_voxel=5, use_rotate_nms=True, num_point_features=4)),
    ("all.fhd.config", "ALL_FHD_KITTI", [1, 160, 132],          # KITTI, four classes: SimpleVoxelRadius + SpMiddleFHD(3) + a two-block RPN
     dict(vfe="SimpleVoxelRadius", middle="SpMiddleFHD", middle_in=3, downsample_factor=8, num_anchor_per_loc=8, num_class=4,
          max_points_per_voxel=5, use_rotate_nms=True, num_point_features=4)),
]


@pytest.fixture(scope="module")
def ref():
    if not os.path.isdir(os.path.join(REF, "second")):
        pytest.skip("reference checkout not present")
    from second_amd import compat
    compat.install(REF)
    import second.pytorch.train as train
    return train


def _model_cfg(rel, pre_max=None):
    from google.protobuf import text_format
    from second.protos import pipeline_pb2
    cfg = pipeline_pb2.TrainEvalPipelineConfig()
    text_format.Merge(open(os.path.join(REF, "second/configs", rel)).read(), cfg)
    if pre_max:
        for cs in cfg.model.second.target_assigner.class_settings:
            cs.nms_pre_max_size = pre_max                          # keeps the pure-Python iou_jit fast
    return cfg.model.second


def _example_of(train, net, clouds, max_voxels, fm):
    vox = [net.voxel_generator.generate(c, max_voxels) for c in clouds]
    anchors = net.target_assigner.generate_anchors(list(fm))["anchors"].reshape(1, -1, 7)
    example = {
        "voxels": np.concatenate([v["voxels"] for v in vox]),
        "num_points": np.concatenate([v["num_points_per_voxel"] for v in vox]),
        "coordinates": np.concatenate([np.pad(v["coordinates"], ((0, 0), (1, 0)), mode="constant", constant_values=b)
                                       for b, v in enumerate(vox)]),
        "anchors": np.repeat(anchors, len(clouds), 0),
        "metadata": [{"image_idx": 10 + b} for b in range(len(clouds))],
    }
    return train.example_convert_to_torch(example, torch.float32, torch.device("cpu"))


@pytest.mark.parametrize("rel, name, fm, want_cfg", CASES)
def test_accelerate_model_serves_the_reference_lite_and_people_networks(ref, rel, name, fm, want_cfg):
    import oracle_backend
    from lite_helpers import clouds_for, trained_like
    from second_amd import compat, dropin, models
    train = ref
    mcfg = dict(getattr(models, name), nms_pre_max_size=150)
    clouds = clouds_for(mcfg, range(2))
    with oracle_backend.installed():
        net = train.build_network(_model_cfg(rel, 150)).eval()
        c = dropin.model_config(net)
        for k, v in want_cfg.items():
            assert c.get(k) == v, (k, c.get(k), v)
        if "vfe" not in want_cfg:
            assert "vfe" not in c
        like = trained_like(mcfg, clouds[0])                       # distinct scores: no tie-order dependence
        missing = net.load_state_dict(like.state_dict(), strict=False)
        assert not [k for k in missing.missing_keys if k.split(".")[0] in ("middle_feature_extractor", "rpn")]
        np.testing.assert_allclose(like.anchors.numpy(), net.target_assigner.generate_anchors(fm)["anchors"].reshape(-1, 7), rtol=0, atol=1e-5)
        ex = _example_of(train, net, clouds, mcfg["max_voxels"], fm)
        with torch.no_grad():
            want = net(ex)
        assert sum(w["box3d_lidar"].shape[0] for w in want) >= 4
        assert compat.accelerate_model(net) is net
        eng = net._second_amd_engine
        assert eng.cfg["middle"] == want_cfg["middle"] and eng.cfg["nms_pre_max_size"] == 150
        with torch.no_grad():
            got = net(ex)
        assert eng.stats["fused_calls"] == 1 and eng.stats["original_calls"] == 0 and eng.stats["adoptions"] == 1
        assert eng._det.feature_map_size == fm
        assert isinstance(got, list) and len(got) == 2
        for g, w in zip(got, want):
            assert set(g) == set(w) and g["metadata"] == w["metadata"]
            assert g["box3d_lidar"].dtype == w["box3d_lidar"].dtype == torch.float32 and g["label_preds"].dtype == w["label_preds"].dtype
            assert g["scores"].shape == w["scores"].shape
            np.testing.assert_allclose(g["scores"].numpy(), w["scores"].numpy(), rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(g["box3d_lidar"].numpy(), w["box3d_lidar"].numpy(), rtol=1e-4, atol=1e-4)
            np.testing.assert_array_equal(g["label_preds"].numpy(), w["label_preds"].numpy())
        net.train()
        assert not eng.accepts(ex)
        net.eval()


@pytest.mark.parametrize("rel, name, fm, want_cfg", CASES)
def test_lite_standins_are_shaped_like_the_reference_networks(ref, rel, name, fm, want_cfg):
    """tests/reference_standin_lite.py against the real build_network result: same sub-module type names, same state-dict keys and
    shapes, and dropin.model_config reads the SAME configuration from both objects."""
    import oracle_backend
    import reference_standin_lite
    from second_amd import dropin, models
    train = ref
    with oracle_backend.installed():
        real = train.build_network(_model_cfg(rel)).eval()
        mcfg = dict(getattr(models, name), max_voxels=int(real.voxel_generator._max_voxels))
        fake = reference_standin_lite.build_voxelnet_lite(mcfg).eval()
    for part in ("voxel_feature_extractor", "middle_feature_extractor", "rpn"):
        assert type(getattr(real, part)).__name__ == type(getattr(fake, part)).__name__
    rs, fs = real.state_dict(), fake.state_dict()
    keys = lambda sd: {k: tuple(v.shape) for k, v in sd.items() if k.split(".")[0] in ("voxel_feature_extractor", "middle_feature_extractor", "rpn")}
    assert keys(rs) == keys(fs)
    c_real, c_fake = dropin.model_config(real), dropin.model_config(fake)
    c_real.pop("name"), c_fake.pop("name")
    assert set(c_real) == set(c_fake)
    for k in c_real:
        if isinstance(c_real[k], list) and c_real[k] and isinstance(c_real[k][0], float):
            np.testing.assert_allclose(c_fake[k], c_real[k], rtol=1e-6, err_msg=k)
        else:
            assert c_fake[k] == c_real[k], (k, c_fake[k], c_real[k])
    # the mirror restates the config file's grid and thresholds
    for k in ("point_cloud_range", "voxel_size", "post_center_range"):
        np.testing.assert_allclose(getattr(models, name)[k], c_real[k], rtol=1e-6, err_msg=k)
    for k in ("nms_score_threshold", "nms_iou_threshold", "nms_pre_max_size", "nms_post_max_size", "direction_limit_offset", "direction_offset"):
        assert abs(getattr(models, name)[k] - c_real[k]) < 1e-6, k


def test_mismatched_vfe_and_middle_are_refused_with_the_reason(ref):
    """A middle whose first conv does not take what the VFE produces is named, not served."""
    import oracle_backend
    from second_amd import compat, dropin
    mc = _model_cfg("car.lite.config")
    mc.voxel_feature_extractor.module_class_name = "SimpleVoxel"           # four channels into SpMiddleFHDLite(3)
    with oracle_backend.installed():
        net = ref.build_network(mc).eval()
    with pytest.raises(dropin.NotAccelerable, match="SpMiddleFHDLite takes 3 input channels, SimpleVoxel produces 4"):
        dropin.model_config(net)
    assert compat.accelerate_model(net, strict=False) is net and getattr(net, "_second_amd_engine", None) is None


def test_a_second_install_keeps_the_proto_message_classes(ref):
    """compat.install() is idempotent for the reference's protos: modules of the reference imported after the first call
    (second/builder/voxel_builder.py) hold the first set of message classes and check their arguments with isinstance, so a later
    install() -- another test module's fixture, a launcher called twice -- must hand back the same classes, not rebuilt ones."""
    import sys
    from second_amd import compat
    mod = sys.modules["second.protos.voxel_generator_pb2"]
    cls, pipe = mod.VoxelGenerator, sys.modules["second.protos.pipeline_pb2"].TrainEvalPipelineConfig
    names = compat.install(REF)
    assert "voxel_generator_pb2" in names and "pipeline_pb2" in names
    assert sys.modules["second.protos.voxel_generator_pb2"] is mod and mod.VoxelGenerator is cls
    assert sys.modules["second.protos.pipeline_pb2"].TrainEvalPipelineConfig is pipe
    from second.builder import voxel_builder
    vg = voxel_builder.build(_model_cfg("car.lite.config").voxel_generator)          # the isinstance check that a rebuilt class fails
    assert vg.grid_size.tolist() == [1056, 1280, 40]
