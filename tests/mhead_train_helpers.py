"""Shared by tests/test_mhead_train_host.py, tests/test_gpu_mhead_train.py and tests/test_dropin_reference_mhead_train.py: the
reduced geometry of nuscenes/all.pp.mhead the trainer tests run at, a fixed synthetic batch for it, and ragged pillars for the
PillarFeatureNetRadius training kernels."""
import numpy as np
import torch

RANGE, VOXEL = (-50.0, -50.0, -5.0, 50.0, 50.0, 3.0), (0.25, 0.25, 8.0)


def small_cfg(**over):
    """all.pp.mhead at +-10 m: 80 x 80 pillars, trunk map 20 x 20 (large head), block 0's 40 x 40 cropped by 4 to 32 x 32 (small
    head); anchors +-10 m for the large classes and +-8 m for the small ones: 4 800 + 8 192 anchors (tests/golden/mhead.npz)."""
    from second_amd.models import ALL_PP_MHEAD as c
    lim = lambda r: [(-8.0 if v == -40 else 8.0 if v == 40 else -10.0 if v == -50 else 10.0 if v == 50 else v) for v in r]
    cfg = dict(c, point_cloud_range=[-10, -10, -5, 10, 10, 3], anchor_ranges=[lim(r) for r in c["anchor_ranges"]],
               group_feature_map_sizes=[[1, 20, 20]] * 5 + [[1, 32, 32]] * 5, max_voxels=6400,
               heads=[dict(c["heads"][0], feature_map_size=[1, 20, 20]), dict(c["heads"][1], feature_map_size=[1, 32, 32])])
    cfg.update(over)
    return cfg


GT_CLASSES = (1, 2, 5, 6, 7, 9, 10, 2, 9, 6)       # per frame: three classes of the large head, four of the small one


def small_batch(det, frames=2, points=8000, seed=0):
    """(points, point_offsets, gt_boxes, gt_offsets, gt_classes) as numpy arrays: ``points`` uniform points per frame, ten boxes per
    frame -- GT_CLASSES, each an anchor of its class with the centre inside +-8 m, nudged by a few centimetres."""
    from second_amd.models import anchor_class_ranges
    rng = np.random.default_rng(seed)
    begin = anchor_class_ranges(det.cfg, det.feature_map_size)
    anc = det.anchors.cpu().numpy()
    pts, offs, gts, goffs, gcls = [], [0], [], [0], []
    for _ in range(frames):
        p = rng.uniform([-9.9, -9.9, -4.9, 0], [9.9, 9.9, 2.9, 1], (points, 4)).astype(np.float32)
        pts.append(p)
        offs.append(offs[-1] + len(p))
        boxes = []
        for c in GT_CLASSES:
            seg = anc[begin[c - 1]:begin[c]]
            seg = seg[(np.abs(seg[:, 0]) < 7.5) & (np.abs(seg[:, 1]) < 7.5)]
            boxes.append(seg[rng.integers(len(seg))])
        b = np.stack(boxes).astype(np.float32)
        b[:, :2] += rng.normal(0, 0.03, (len(b), 2)).astype(np.float32)
        assert np.abs(b[:, :2]).max() < 8.0
        gts.append(b)
        goffs.append(goffs[-1] + len(b))
        gcls.append(np.array(GT_CLASSES, np.int32))
    return (np.concatenate(pts), np.array(offs, np.int32), np.concatenate(gts), np.array(goffs, np.int32), np.concatenate(gcls))


def ragged_pillars(p, t, seed):
    """[P, T, 4] pillars of the all.pp.mhead grid with 1 .. T points (every seventh pillar full), points inside their pillar;
    pillar 0 is the one whose corner is the sensor axis and its first point lies exactly at x = y = 0 (radius 0)."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(1, t + 1, (p,), generator=g)
    n[::7] = t
    cy, cx = torch.randint(0, 400, (p,), generator=g), torch.randint(0, 400, (p,), generator=g)
    cy[0], cx[0] = 200, 200
    coors = torch.stack([torch.zeros(p, dtype=torch.long), torch.zeros(p, dtype=torch.long), cy, cx], 1).int()
    vox = torch.zeros(p, t, 4)
    vox[..., 0] = RANGE[0] + (cx.view(-1, 1) + torch.rand(p, t, generator=g) * 0.96 + 0.02) * VOXEL[0]
    vox[..., 1] = RANGE[1] + (cy.view(-1, 1) + torch.rand(p, t, generator=g) * 0.96 + 0.02) * VOXEL[1]
    vox[..., 2] = torch.rand(p, t, generator=g) * 4 - 3
    vox[..., 3] = torch.rand(p, t, generator=g)
    vox[0, 0, 0] = vox[0, 0, 1] = 0.0
    vox *= (torch.arange(t).view(1, -1) < n.view(-1, 1)).unsqueeze(-1)
    return vox, n.int(), coors
