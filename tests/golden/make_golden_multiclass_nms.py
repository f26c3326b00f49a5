"""Produces tests/golden/multiclass_nms.npz by EXECUTING the reference's own ``VoxelNet.predict`` (voxelnet.py:377-645) on the CPU
with ``_multiclass_nms = True``.  Build container only (needs the reference checkout and the built CPU oracle):

    python tests/golden/make_golden_multiclass_nms.py [path to the reference checkout]

The method runs unbound on a stand-in that carries exactly the attributes it reads; box coder, target assigner and anchor generators
are the reference's own objects, box_torch_ops.rotate_nms / nms its own functions (their compiled leaf, spconv's
rotate_non_max_suppression_cpu / non_max_suppression, is this repository's CPU oracle, as in tests/test_dropin_reference.py).
Geometry, per-class settings and cases: tests/multiclass_nms_helpers.py.  Asserted here, per case and frame (another seed is tried
until all hold -- nothing is excluded at test time):
  * the scores of a class's candidates are pairwise distinct (torch.topk's tie order is unspecified);
  * no candidate pair's IoU lies within IOU_MARGIN of its class's threshold;
  * class 0 has more candidates than its pre_max, class 1 more than 1 024 passing anchors (class-agnostic cases), class 2 no candidate
    on frame 1, a class is cut by its post_max, a box falls outside post_center_range, every frame keeps something."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def logits(seed):
    """cls [B, A, H, W, C] float32: a -6 floor, class 0 and 2 sparse bumps (class 2 none on frame 1), class 1 broad."""
    import multiclass_nms_helpers as M
    rng = np.random.default_rng(seed)
    n = M.A * M.H * M.W
    cls = np.full((M.B, n, M.C), -6.0, np.float32)
    own = lambda c: np.arange(2 * c * M.H * M.W, (2 * c + 2) * M.H * M.W)
    for b in range(M.B):
        for c, (n_own, n_else) in ((0, (30, 30)), (2, (12, 12))):
            if c == 2 and b == 1:
                continue
            idx = np.concatenate([rng.choice(own(c), n_own, replace=False), rng.choice(np.setdiff1d(np.arange(n), own(c)), n_else, replace=False)])
            cls[b, idx, c] = rng.normal(1.0, 1.0, len(idx)).astype(np.float32)
        cls[b, :, 1] = rng.normal(-2.0, 2.0, n).astype(np.float32)
    box = (rng.normal(0, 0.25, (M.B, n, 7))).astype(np.float32)
    dirs = rng.normal(0, 1, (M.B, n, 2)).astype(np.float32)
    r5 = lambda t: np.ascontiguousarray(t.reshape(M.B, M.A, M.H, M.W, -1))
    return r5(cls), r5(box), r5(dirs)


def pair_ious(boxes, dets, rotate):
    """IoU of every candidate pair as the NMS of that kind measures it."""
    from oracle import oracle as orc
    if rotate:
        return orc.rotate_iou(dets[:, :5].astype(np.float32), dets[:, :5].astype(np.float32))
    x1, y1, x2, y2 = (dets[:, i].astype(np.float64) for i in range(4))
    w = np.maximum(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]) + 1, 0)
    h = np.maximum(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]) + 1, 0)
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    return w * h / (area[:, None] + area[None] - w * h)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SECOND_REFERENCE", "/root/reference")
    sys.path[:0] = [os.path.join(ROOT, "second.pytorch_amd"), ROOT, os.path.join(ROOT, "tests")]
    import torch
    import multiclass_nms_helpers as M
    import oracle_backend
    from second_amd import compat, models
    compat.install(ref)
    from second.core import region_similarity
    from second.core.anchor_generator import AnchorGeneratorRange
    from second.core.target_assigner import TargetAssigner
    from second.pytorch.core import box_torch_ops
    from second.pytorch.core.box_coders import GroundBox3dCoderTorch
    from second.pytorch.models.voxelnet import VoxelNet

    cfg0 = M.config()
    fm = [1, M.H, M.W]
    names = ["Car", "Cyclist", "Pedestrian"]
    gens = [AnchorGeneratorRange(anchor_ranges=r, sizes=s, rotations=cfg0["rotations"], class_name=nm, match_threshold=mt, unmatch_threshold=ut)
            for r, s, nm, mt, ut in zip(cfg0["anchor_ranges"], cfg0["anchor_sizes"], names, cfg0["matched_thresholds"], cfg0["unmatched_thresholds"])]
    coder = GroundBox3dCoderTorch()
    ta = TargetAssigner(coder, gens, names, feature_map_sizes=[fm] * 3, positive_fraction=None,
                        region_similarity_calculators=[region_similarity.NearestIouSimilarity() for _ in gens], sample_size=512)
    anchors = ta.generate_anchors(fm)["anchors"].reshape(-1, 7).astype(np.float32)
    assert np.array_equal(anchors, models.generate_anchors(cfg0, fm)), "models.generate_anchors is not the reference's generator"
    begin = models.anchor_class_ranges(cfg0, fm)
    assert [tuple(int(v) for v in ta.anchors_range(c)) for c in range(M.C)] == list(zip(begin[:-1], begin[1:]))
    assert ta.num_anchors_per_location == M.A

    def standin(rotate, agnostic):
        cfg = M.config(rotate, agnostic)
        return types.SimpleNamespace(
            _box_coder=coder, _num_class=M.C, _encode_background_as_zeros=True, _use_sigmoid_score=True, _use_direction_classifier=True,
            _num_direction_bins=cfg["num_direction_bins"], _post_center_range=cfg["post_center_range"], _use_rotate_nms=rotate,
            target_assigner=ta, _multiclass_nms=True, _nms_class_agnostic=agnostic, _nms_score_thresholds=list(M.THR),
            _nms_pre_max_sizes=list(M.PRE), _nms_post_max_sizes=list(M.POST), _nms_iou_thresholds=list(M.IOU),
            _dir_offset=cfg["direction_offset"], _dir_limit_offset=cfg["direction_limit_offset"])

    def check_and_run(seed):
        """-> (inputs, {case: [frame outputs]}) or a string saying which property the seed misses."""
        cls, box, dirs = logits(seed)
        n = M.A * M.H * M.W
        example = {"anchors": torch.from_numpy(anchors).unsqueeze(0).repeat(M.B, 1, 1)}
        preds = {"cls_preds": torch.from_numpy(cls), "box_preds": torch.from_numpy(box), "dir_cls_preds": torch.from_numpy(dirs)}
        scores = torch.sigmoid(torch.from_numpy(cls).reshape(M.B, n, M.C)).numpy()
        dec = coder.decode_torch(torch.from_numpy(box).reshape(M.B, n, 7), example["anchors"])
        res = {}
        for name, (rotate, agnostic) in M.CASES.items():        # the cheap properties of every case first
            for b in range(M.B):
                for c in range(M.C):
                    lo, hi = (0, n) if agnostic else (begin[c], begin[c + 1])
                    s = scores[b, lo:hi, c]
                    cand = np.flatnonzero(s >= np.float32(M.THR[c]))
                    if len(np.unique(s[cand])) != len(cand):
                        return f"{name}: equal candidate scores (frame {b}, class {c})"
                    if c == 0 and len(cand) <= M.PRE[0]:
                        return f"{name}: class 0 has no more candidates than its pre_max"
                    if c == 1 and agnostic and len(cand) <= 1024:
                        return f"{name}: class 1 has only {len(cand)} passing anchors"
                    if c == 2 and b == 1 and len(cand):
                        return f"{name}: class 2 has candidates on frame 1"
                    top = cand[np.argsort(-s[cand], kind="stable")][:M.PRE[c]]
                    if len(top) < 2:
                        continue
                    bx = dec[b, lo:hi][top]
                    nb = bx[:, [0, 1, 3, 4, 6]]
                    if not rotate:
                        nb = box_torch_ops.corner_to_standup_nd(box_torch_ops.center_to_corner_box2d(nb[:, :2], nb[:, 2:4], nb[:, 4]))
                    iou = pair_ious(bx.numpy(), nb.numpy(), rotate)
                    off = np.abs(iou - M.IOU[c])[np.triu_indices(len(top), 1)]
                    if off.min() < M.IOU_MARGIN:
                        return f"{name}: a pair's IoU within {M.IOU_MARGIN} of the threshold (frame {b}, class {c})"
        for name, (rotate, agnostic) in M.CASES.items():
            cut_by_post = False
            with torch.no_grad(), oracle_backend.installed():
                out = VoxelNet.predict(standin(rotate, agnostic), dict(example), {k: v.clone() for k, v in preds.items()})
            frames = []
            for b, o in enumerate(out):
                lab = o["label_preds"].numpy()
                if len(lab) == 0:
                    return f"{name}: frame {b} keeps nothing"
                frames.append({"boxes": o["box3d_lidar"].numpy().astype(np.float32), "scores": o["scores"].numpy().astype(np.float32),
                               "labels": lab.astype(np.int64)})
            # the same call without the range mask: which boxes fall outside, and which class fills its post_max
            free = standin(rotate, agnostic)
            free._post_center_range = []
            with torch.no_grad(), oracle_backend.installed():
                unmasked = VoxelNet.predict(free, dict(example), {k: v.clone() for k, v in preds.items()})
            outside = sum(len(u["label_preds"]) - len(o["label_preds"]) for u, o in zip(unmasked, out))
            if outside < 1:
                return f"{name}: no box outside post_center_range"
            for u in unmasked:
                cnt = np.bincount(u["label_preds"].numpy(), minlength=M.C)
                cut_by_post |= bool((cnt[[0, 2]] == np.array(M.POST)[[0, 2]]).any())
            if not cut_by_post:
                return f"{name}: no class is cut by its post_max"
            print(name, "seed", seed, "kept per frame", [len(f["labels"]) for f in frames], "outside the range", outside,
                  "labels", [np.bincount(f["labels"], minlength=M.C).tolist() for f in frames])
            res[name] = frames
        return (cls, box, dirs), res

    for seed in range(100, 500):
        got = check_and_run(seed)
        if not isinstance(got, str):
            break
        print("seed", seed, "rejected:", got)
    else:
        raise SystemExit("no seed satisfies the fixture's properties")
    (cls, box, dirs), res = got
    out = {"cls": cls, "box": box, "dir": dirs}
    for name, frames in res.items():
        for f, fr in enumerate(frames):
            for k, v in fr.items():
                out[f"{name}/f{f}/{k}"] = v
    out["meta"] = np.array(json.dumps({"seed": seed, "pre": M.PRE, "post": M.POST, "thr": M.THR, "iou": M.IOU, "iou_margin": M.IOU_MARGIN,
                                       "H": M.H, "W": M.W, "A": M.A, "C": M.C, "B": M.B}))
    path = os.path.join(HERE, "multiclass_nms.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
