"""Shared by the multi-class NMS tests and tests/golden/make_golden_multiclass_nms.py: the small three-class detector configuration
of the fixture, its cases, and the reading of tests/golden/multiclass_nms.npz."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multiclass_nms.npz")

# three classes x 2 rotations on a 16 x 24 map: 6 anchors per location, 2 304 anchors, class c owns a in [2c, 2c + 2)
H, W, A, C, B = 16, 24, 6, 3, 2
PRE, POST = (16, 1024, 7), (4, 100, 3)
THR, IOU = (0.3, 0.05, 0.4), (0.3, 0.5, 0.1)
# |IoU - iou_c| of every candidate pair of the fixture stays above this: the 2e-5 the NMS fixtures' IoU values are held to
# (tests/golden/make_golden.py; fp32 rounding of an IoU is ~1e-6), so no keep decision hangs on rounding
IOU_MARGIN = 2e-5
CASES = {"rot_ranges": (True, False), "rot_agnostic": (True, True), "aa_ranges": (False, False), "aa_agnostic": (False, True)}


def config(rotate=True, agnostic=False, multiclass=True):
    """SecondDetector configuration of the fixture's geometry (car.fhd's network on a 19.2 m x 12.8 m range, KITTI all.fhd's first
    three anchor classes)."""
    from second_amd import models as M
    cfg = dict(M.CAR_FHD, name="multiclass_nms.fixture",
               point_cloud_range=[0, -6.4, -3, 19.2, 6.4, 1], voxel_size=[0.1, 0.1, 0.1], max_voxels=4000,
               anchor_sizes=[[1.6, 3.9, 1.56], [0.6, 1.76, 1.73], [0.6, 0.8, 1.73]],
               anchor_ranges=[[0, -6.4, z, 19.2, 6.4, z] for z in (-1.0, -0.6, -0.6)],
               matched_thresholds=[0.6, 0.35, 0.35], unmatched_thresholds=[0.45, 0.2, 0.2], num_class=C,
               use_rotate_nms=bool(rotate), post_center_range=[1.0, -5.5, -2.2, 18.0, 5.5, 0.8])
    if multiclass:
        cfg.update(multiclass_nms=True, nms_class_agnostic=bool(agnostic), nms_score_thresholds=list(THR), nms_pre_max_sizes=list(PRE),
                   nms_post_max_sizes=list(POST), nms_iou_thresholds=list(IOU))
    return cfg


def load():
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    fx = {"meta": meta, "cls": z["cls"], "box": z["box"], "dir": z["dir"], "cases": {}}
    for name in CASES:
        frames = []
        for f in range(B):
            frames.append({k: z[f"{name}/f{f}/{k}"] for k in ("boxes", "scores", "labels")})
        fx["cases"][name] = frames
    return fx


def preds_of(fx, dtype=None, device=None):
    """The head tensors as the RPN returns them: [B, A, H, W, code] (anchor n = (a * H + y) * W + x)."""
    import torch
    out = {}
    for k, name in (("cls_preds", "cls"), ("box_preds", "box"), ("dir_cls_preds", "dir")):
        t = torch.from_numpy(fx[name])
        if dtype is not None:
            t = t.to(dtype)
        out[k] = t.to(device) if device is not None else t
    return out
