"""Shared by tests/golden/make_golden_anchor_mask.py, tests/test_anchor_mask_host.py and tests/test_gpu_anchor_mask.py: the cases of
tests/golden/anchor_mask.npz, a vectorised numpy float32 restatement of the reference's ``anchors_mask``
(second/data/preprocess.py:345-357 over box_np_ops.rbbox2d_to_near_bbox :286-298, sparse_sum_for_anchors_mask :917-922 and
fused_get_anchors_area :925-946) and a torch restatement of the masked ``VoxelNet.predict`` (voxelnet.py:429-439).  Nothing here
calls the device kernels under test."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_mask.npz")
CAR, PED = [1.6, 3.9, 1.56], [0.6, 0.8, 1.73]

# geometry of every case: anchor_generator_stride settings per class (class-major anchor array, like target_assigner.generate_anchors)
CASES = {
    # xyres_16 cells on a 64 x 64 grid, 2 048 anchors
    "A": dict(pc_range=[0, -5.12, -3, 10.24, 5.12, 1], voxel_size=[0.16, 0.16, 4], fm=[1, 32, 32], thresholds=[0, 1, 5], frames=3,
              classes=[dict(name="Car", sizes=CAR, strides=[0.32, 0.32, 0.0], offsets=[0.16, -4.96, -1.78], rotations=[0, 1.57],
                            matched=0.6, unmatched=0.45)]),
    # a 3-D grid (8 cells high) whose BEV map is 40 x 72: counts above 1, a width that is no multiple of 64, two classes
    "B": dict(pc_range=[0, -4, -3, 14.4, 4, 1], voxel_size=[0.2, 0.2, 0.5], fm=[1, 20, 36], thresholds=[0, 1, 4], frames=3,
              classes=[dict(name="Car", sizes=CAR, strides=[0.4, 0.4, 0.0], offsets=[0.2, -3.8, -1.0], rotations=[0, 1.57],
                            matched=0.6, unmatched=0.45),
                       dict(name="Pedestrian", sizes=PED, strides=[0.4, 0.4, 0.0], offsets=[0.2, -3.8, -0.6], rotations=[0, 1.57],
                            matched=0.5, unmatched=0.35)]),
    # the full xyres_16 geometry: 432 x 496 cells, 107 136 anchors
    "C": dict(pc_range=[0, -39.68, -3, 69.12, 39.68, 1], voxel_size=[0.16, 0.16, 4], fm=[1, 248, 216], thresholds=[1], frames=2,
              classes=[dict(name="Car", sizes=CAR, strides=[0.32, 0.32, 0.0], offsets=[0.16, -39.52, -1.78], rotations=[0, 1.57],
                            matched=0.6, unmatched=0.45)]),
}


def geometry(case):
    """-> (voxel_size float32 [3], pc_range float32 [6], grid (nx, ny, nz)) as the voxel generator keeps them."""
    vs, rng = np.array(case["voxel_size"], np.float32), np.array(case["pc_range"], np.float32)
    return vs, rng, np.round((rng[3:] - rng[:3]) / vs).astype(np.int64)


def anchors_of(case):
    """-> (anchors [A, 7] float32 ordered (class, size x rotation, z, y, x), begin of every class's range + the total)."""
    d, h, w = case["fm"]
    out, begin = [], [0]
    for c in case["classes"]:
        zc = np.arange(d, dtype=np.float32) * c["strides"][2] + c["offsets"][2]
        yc = np.arange(h, dtype=np.float32) * c["strides"][1] + c["offsets"][1]
        xc = np.arange(w, dtype=np.float32) * c["strides"][0] + c["offsets"][0]
        rots = np.array(c["rotations"], np.float32)
        a = np.zeros((1, len(rots), d, h, w, 7), np.float32)
        a[..., 0], a[..., 1], a[..., 2] = xc[None, None, None, None, :], yc[None, None, None, :, None], zc[None, None, :, None, None]
        a[..., 3:6] = np.array(c["sizes"], np.float32)
        a[..., 6] = rots[None, :, None, None, None]
        out.append(a.reshape(-1, 7))
        begin.append(begin[-1] + len(out[-1]))
    return np.concatenate(out), begin


def near_bbox_np(anchors):
    """rbbox2d_to_near_bbox(anchors[:, [0, 1, 3, 4, 6]]) in float32."""
    a = np.asarray(anchors, np.float32)
    pi = np.float32(np.pi)
    r = a[:, 6]
    lim = r - np.floor(r / pi + np.float32(0.5)) * pi
    swap = np.abs(lim) > np.float32(np.pi / 4)
    dx, dy = np.where(swap, a[:, 4], a[:, 3]), np.where(swap, a[:, 3], a[:, 4])
    two = np.float32(2)
    return np.stack([a[:, 0] - dx / two, a[:, 1] - dy / two, a[:, 0] + dx / two, a[:, 1] + dy / two], 1).astype(np.float32)


def anchor_cells(anchors, voxel_size, pc_range, grid, dtype=np.float32):
    """The four cell indices per anchor [A, 4] (c0, c1, c2, c3), clamped to the map on both sides; ``dtype`` = the arithmetic of the
    four quotients (float32: the reference's; float64 on the same float32 inputs: what the fixture's teeth are measured against)."""
    bv = near_bbox_np(anchors).astype(dtype)
    vs, off = np.asarray(voxel_size, np.float32).astype(dtype), np.asarray(pc_range, np.float32).astype(dtype)
    c = np.stack([np.floor((bv[:, 0] - off[0]) / vs[0]), np.floor((bv[:, 1] - off[1]) / vs[1]),
                  np.floor((bv[:, 2] - off[0]) / vs[0]), np.floor((bv[:, 3] - off[1]) / vs[1])], 1)
    assert c.dtype == dtype
    c = c.astype(np.int64)
    c[:, [0, 2]] = np.clip(c[:, [0, 2]], 0, int(grid[0]) - 1)
    c[:, [1, 3]] = np.clip(c[:, [1, 3]], 0, int(grid[1]) - 1)
    return c


def anchor_mask_np(coors_zyx, anchors, voxel_size, pc_range, grid, threshold, dtype=np.float32):
    """bool [A]: the frame's anchors_mask.  coors_zyx [M, 3] integer voxel coordinates of ONE frame."""
    nx, ny = int(grid[0]), int(grid[1])
    dense = np.zeros((ny, nx), np.int64)
    if len(coors_zyx):
        np.add.at(dense, (np.asarray(coors_zyx)[:, 1].astype(np.int64), np.asarray(coors_zyx)[:, 2].astype(np.int64)), 1)
    dense = dense.cumsum(0).cumsum(1)
    c = anchor_cells(anchors, voxel_size, pc_range, grid, dtype)
    # the reference's arithmetic: the row and the column of the MIN cell are excluded (no "- 1")
    area = dense[c[:, 3], c[:, 2]] - dense[c[:, 3], c[:, 0]] - dense[c[:, 1], c[:, 2]] + dense[c[:, 1], c[:, 0]]
    return area > threshold


def batch_mask_np(coors_bzyx, batch, anchors, voxel_size, pc_range, grid, threshold):
    """uint8 [B, A] from batched coordinates [M, 4] (b, z, y, x)."""
    co = np.asarray(coors_bzyx)
    return np.stack([anchor_mask_np(co[co[:, 0] == b][:, 1:], anchors, voxel_size, pc_range, grid, threshold) for b in range(batch)]).astype(np.uint8)


def load_case(z, name):
    """-> dict(coors [list per frame of [M, 3] int], masks {threshold: bool [frames, A]}) of the fixture ``z``."""
    case = CASES[name]
    a = len(anchors_of(case)[0])
    coors = [z[f"{name}_coors_{f}"].astype(np.int32) for f in range(case["frames"])]
    masks = {t: np.unpackbits(z[f"{name}_mask_t{t}"], axis=1)[:, :a].astype(bool) for t in case["thresholds"]}
    return dict(coors=coors, masks=masks)


def masked_predict_torch(net, preds, anchors, masks):
    """voxelnet.py:429-439: index the frame's head rows and anchors by its mask, then the un-masked torch formulation of predict
    (``net.fused_predict`` off) on that frame alone.  preds: head tensors [B, ...]; anchors [A, 7]; masks [B, A].  -> list of dicts."""
    import torch
    b = masks.shape[0]
    was, net.fused_predict = net.fused_predict, False
    res = []
    try:
        for f in range(b):
            idx = torch.nonzero(masks[f] != 0).flatten()
            if idx.numel() == 0:
                dev = anchors.device
                res.append({"box3d_lidar": torch.zeros((0, 7), device=dev), "scores": torch.zeros((0,), device=dev),
                            "label_preds": torch.zeros((0,), dtype=torch.int64, device=dev), "metadata": None})
                continue
            codes = {"box_preds": 7, "cls_preds": net.cfg["num_class"], "dir_cls_preds": net.cfg["num_direction_bins"]}
            pf = {k: preds[k][f].float().reshape(1, -1, c)[:, idx].contiguous() for k, c in codes.items() if k in preds}
            r = net.predict(pf, anchors[idx].unsqueeze(0).float().contiguous())[0]
            r["label_preds"] = r["label_preds"].long()
            res.append(r)
    finally:
        net.fused_predict = was
    return res
