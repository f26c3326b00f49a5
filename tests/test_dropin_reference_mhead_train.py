"""Training-mode drop-in check for ``nuscenes/all.pp.mhead.config`` (build container only: needs the reference checkout), in the
manner of tests/test_dropin_reference_mhead.py: the UNMODIFIED reference network at the reduced geometry of the trainer tests, in
train(), against ``SecondDetector(cfg).train()`` on the same state: one forward of each on the same example gives the same
predictions and leaves the same running statistics in EVERY BatchNorm -- the small head's tower keeps torch's default eps 1e-5 /
momentum 0.1 where every other norm of the network has 1e-3 / 0.01.  CPU, oracle backend."""
import os

import numpy as np
import pytest
import torch

from mhead_train_helpers import small_cfg

REF = os.environ.get("SECOND_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def ref():
    if not os.path.isdir(os.path.join(REF, "second")):
        pytest.skip("reference checkout not present")
    from second_amd import compat
    compat.install(REF)
    import second.pytorch.train as train
    return train


def _small_model_cfg():
    from google.protobuf import text_format
    from second.protos import pipeline_pb2
    cfg = pipeline_pb2.TrainEvalPipelineConfig()
    text_format.Merge(open(os.path.join(REF, "second/configs/nuscenes/all.pp.mhead.config")).read(), cfg)
    m = cfg.model.second
    m.voxel_generator.point_cloud_range[:] = [-10, -10, -5, 10, 10, 3]
    m.voxel_generator.max_number_of_points_per_voxel = 60
    for cs in m.target_assigner.class_settings:
        ar = cs.anchor_generator_range.anchor_ranges
        small = abs(ar[0]) == 40
        lim = 8.0 if small else 10.0
        ar[0], ar[1], ar[3], ar[4] = -lim, -lim, lim, lim
        cs.feature_map_size[:] = [1, 32, 32] if small else [1, 20, 20]
        cs.nms_pre_max_size = 200
    return m


def test_reference_multi_head_network_in_train_mode_matches_the_mirror(ref):
    import oracle_backend
    from second_amd import synthetic as syn
    from second_amd.models import SecondDetector
    train = ref
    torch.manual_seed(0)
    with oracle_backend.installed():
        net = train.build_network(_small_model_cfg()).train()
        assert type(net).__name__ == "VoxelNetNuscenesMultiHead"
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                    m.running_mean.copy_(torch.empty_like(m.running_mean).uniform_(-0.1, 0.1, generator=g))
                    m.running_var.copy_(torch.empty_like(m.running_var).uniform_(0.5, 1.5, generator=g))
        det = SecondDetector(small_cfg(nms_pre_max_size=200)).train()
        theirs = net.state_dict()
        missing = det.load_state_dict({k: v.clone() for k, v in theirs.items() if k in det.state_dict()})
        assert not missing.missing_keys
        cloud = syn.syn_nusc_cloud(0, num_points=8000, point_cloud_range=(-10, -10, -5, 10, 10, 3))
        vox = net.voxel_generator.generate(cloud, 6400)
        anchors = net.target_assigner.generate_anchors([1, 20, 20])["anchors"].reshape(1, -1, 7)
        assert anchors.shape == (1, 4800 + 8192, 7)
        np.testing.assert_allclose(det.anchors.numpy(), anchors[0], rtol=0, atol=1e-5)
        example = {"voxels": vox["voxels"], "num_points": vox["num_points_per_voxel"],
                   "coordinates": np.pad(vox["coordinates"], ((0, 0), (1, 0)), mode="constant", constant_values=0), "anchors": anchors}
        ex = train.example_convert_to_torch(example, torch.float32, torch.device("cpu"))
        assert net.training and det.training
        ref_preds = net.network_forward(ex["voxels"], ex["num_points"], ex["coordinates"], 1)
        feats = det.voxel_feature_extractor(ex["voxels"], ex["num_points"], ex["coordinates"])
        ours_preds = det.network_forward(feats, ex["coordinates"], 1)
    for k in ("box_preds", "cls_preds", "dir_cls_preds"):
        assert ours_preds[k].shape == ref_preds[k].shape
        np.testing.assert_allclose(ours_preds[k].detach().numpy(), ref_preds[k].detach().numpy(), rtol=1e-3, atol=1e-4)
    # every BatchNorm's buffers after the one forward.  Both sides evaluate torch's own batch_norm on inputs that agree to float32
    # rounding, so the updated statistics agree to a few ulp of float32 sums: rtol 1e-4 (a momentum of 0.01 instead of 0.1, or the
    # reverse, moves a statistic by 9 % of its distance to the batch value -- orders of magnitude more)
    ours, norms = det.state_dict(), 0
    for k, v in net.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert k in ours, k
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(ours[k]) == 1, k
                norms += 1
            else:
                np.testing.assert_allclose(ours[k].numpy(), v.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)
    assert norms == 1 + 4 + 6 + 6 + 3 + 3            # PFN, blocks 0..2, deblocks, the small head's tower
    tower, trunk = dict(net.named_modules())["small_head.net.1"], dict(net.named_modules())["rpn.blocks.0.2"]
    assert (tower.eps, tower.momentum) == (1e-5, 0.1) and (trunk.eps, trunk.momentum) == (1e-3, 0.01)
    assert (det.small_head.net[1].eps, det.small_head.net[1].momentum) == (1e-5, 0.1)
