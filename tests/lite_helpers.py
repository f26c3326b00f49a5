"""Weights and clouds for the tests of the car.lite / people.fhd networks.

tests/e2e_trace.trained_like_detector calibrates the heads through oracle/cpu_forward.forward_frame, which is written for the
SimpleVoxel mean and a one-class label; here the head tensors of the calibration frame come from the detector's OWN CPU
``network_forward`` under the oracle backend, so any VFE / middle / class count the detector can be built with is served."""
import numpy as np
import torch


def clouds_for(cfg, seeds, num_points=6000, num_voxels=5000):
    """syn_kitti_cloud inside ``cfg``'s (smaller) range and voxel grid."""
    from second_amd import synthetic as syn
    return [syn.syn_kitti_cloud(s, num_points=num_points, num_voxels=num_voxels, point_cloud_range=tuple(cfg["point_cloud_range"]),
                                voxel_size=tuple(cfg["voxel_size"])) for s in seeds]


def cpu_example(det, clouds):
    """(voxels, num_points, coordinates with the batch index) of ``clouds`` through the detector's voxel generator, CPU tensors
    (call under oracle_backend.installed())."""
    vox = [det.voxel_generator.generate(c, det.cfg["max_voxels"]) for c in clouds]
    voxels = torch.from_numpy(np.concatenate([v["voxels"] for v in vox]))
    num = torch.from_numpy(np.concatenate([v["num_points_per_voxel"] for v in vox]).astype(np.int32))
    coors = torch.from_numpy(np.concatenate([np.pad(v["coordinates"], ((0, 0), (1, 0)), mode="constant", constant_values=b)
                                             for b, v in enumerate(vox)]).astype(np.int32))
    return voxels, num, coors


def trained_like(cfg, calib_cloud, seed=0):
    """CPU fp32 ``SecondDetector(cfg)`` with the synthetic 'trained-like' weights (second_amd.synthetic): distinct scores, empty
    regions below the score threshold."""
    import oracle_backend
    from second_amd import synthetic as syn
    from second_amd.models import SecondDetector
    torch.manual_seed(seed)
    det = SecondDetector(cfg).eval()
    syn.randomise_like_trained(det, seed=1)
    with oracle_backend.installed(), torch.no_grad():
        voxels, num, coors = cpu_example(det, [calib_cloud])
        feats = det.voxel_feature_extractor(voxels, num, coors)
        preds = det.network_forward(feats, coors, 1)
    syn.sharpen_heads(det, preds["cls_preds"], preds["box_preds"])
    return det
