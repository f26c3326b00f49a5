"""Produces tests/golden/box_custom.npz by EXECUTING the reference on CPU with boxes of nine values (x, y, z, w, l, h, r, vx, vy):
anchor generators with ``custom_values``, ``GroundBox3dCoder(custom_ndim=2)``, ``TargetAssigner.assign`` (assign_per_class and
assign_all), ``second_box_decode`` (torch), ``create_loss`` + ``get_direction_target`` with nine code weights under autograd, and the
box side of ``random_flip`` / ``global_rotation_v2`` / ``global_scaling_v2``.  Build container only (needs the reference checkout):

    python tests/golden/make_golden_box_custom.py [path to the reference checkout]

What the executed reference does with the types (recorded, asserted below): AnchorGeneratorRange with custom values returns FLOAT64
anchors -- its float32 grid widened beside a float64 custom block (anchor_generator.py:57-62) -- and TargetAssigner.assign then
returns float64 bbox_targets.  The loss runs in float64 on purpose (the fixture is the yardstick of a float32 kernel).

Setup: feature map [1, 12, 10]; car (two rotations, nearest IoU, 0.6 / 0.45, custom [0.25, -0.5]), pedestrian (one rotation,
0.5 / 0.35, custom [0, 0]).  Ground truth = jittered anchors with velocities drawn from N(0, 3); frame 0 interleaves the classes,
frame 1 is empty, frame 2 holds cars only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

FM = [1, 12, 10]
CLASSES = ["car", "pedestrian"]
SPEC = [dict(sizes=[1.6, 3.9, 1.56], rotations=[0, 1.57], z=-1.0, mt=0.6, ut=0.45, custom=[0.25, -0.5]),
        dict(sizes=[0.6, 0.8, 1.73], rotations=[0], z=-0.6, mt=0.5, ut=0.35, custom=[0.0, 0.0])]
RANGE_XY = (-4.0, -4.8, 4.0, 4.8)
CODE_WEIGHTS = [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 2.0, 0.25, 1.5]
LOSS = dict(alpha=0.4, gamma=2.0, sigma=2.0, pos_cls_weight=2.0, neg_cls_weight=0.5, classification_weight=1.5, localization_weight=0.7,
            direction_loss_weight=0.3, direction_offset=0.78, sin_error_factor=2.0)
LOSS_ANCHORS = 96
ANGLE, SCALE = 0.3926990816987241, 1.03125          # pi / 8; 33 / 32


def draw_frame(rng, adict, counts):
    g, names = [], []
    for c, k in zip(CLASSES, counts):
        if k == 0:
            continue
        a = np.asarray(adict[c]["anchors"]).reshape(-1, 9)
        b = a[rng.choice(len(a), k, replace=False)].astype(np.float32)
        b[:, :2] += rng.normal(0, 0.12, (k, 2)).astype(np.float32)
        b[:, 3:6] *= rng.uniform(0.92, 1.1, (k, 3)).astype(np.float32)
        b[:, 6] += rng.normal(0, 0.2, k).astype(np.float32)
        b[:, 7:9] = rng.normal(0, 3, (k, 2)).astype(np.float32)
        g.append(b); names += [c] * k
    order = rng.permutation(len(names))
    boxes = np.concatenate(g)[order].astype(np.float32) if g else np.zeros((0, 9), np.float32)
    return boxes, [names[i] for i in order]


def main():
    if len(sys.argv) > 1:
        os.environ["SECOND_REFERENCE"] = sys.argv[1]
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import make_golden
    make_golden.install_shims()
    if not getattr(np.meshgrid, "_as_list", False):
        _mg = np.meshgrid
        np.meshgrid = lambda *a, **k: list(_mg(*a, **k))
        np.meshgrid._as_list = True
    import torch
    from second.core import preprocess, region_similarity
    from second.core.anchor_generator import AnchorGeneratorRange
    from second.core.box_coders import GroundBox3dCoder
    from second.core.target_assigner import TargetAssigner
    from second.pytorch.core import box_torch_ops, losses
    from second.pytorch.models import voxelnet as V

    gens = [AnchorGeneratorRange([RANGE_XY[0], RANGE_XY[1], sp["z"], RANGE_XY[2], RANGE_XY[3], sp["z"]], sizes=sp["sizes"],
                                 rotations=sp["rotations"], class_name=c, match_threshold=sp["mt"], unmatch_threshold=sp["ut"],
                                 custom_values=sp["custom"]) for c, sp in zip(CLASSES, SPEC)]
    coder = GroundBox3dCoder(custom_ndim=gens[0].custom_ndim)
    assert coder.code_size == 9
    assigners = {tag: TargetAssigner(coder, gens, CLASSES, feature_map_sizes=[FM] * 2, positive_fraction=None,
                                     region_similarity_calculators=[region_similarity.NearestIouSimilarity()] * 2, sample_size=512,
                                     assign_per_class=per_class) for tag, per_class in (("per_class", True), ("all", False))}
    ta = assigners["per_class"]
    ret = ta.generate_anchors(FM)
    anchors = ret["anchors"].reshape(-1, 9)
    adict = ta.generate_anchors_dict(FM)
    begin = np.cumsum([0] + [np.asarray(adict[c]["anchors"]).reshape(-1, 9).shape[0] for c in CLASSES]).astype(np.int32)
    assert anchors.dtype == np.float64, anchors.dtype
    a32 = anchors.astype(np.float32)
    assert np.array_equal(a32[:, :7].astype(np.float64), anchors[:, :7]), "columns 0-6 are float32 values widened"
    out = {"feature_map_size": np.array(FM), "anchors": anchors, "class_anchor_begin": begin,
           "matched": np.array([sp["mt"] for sp in SPEC], np.float32), "unmatched": np.array([sp["ut"] for sp in SPEC], np.float32),
           "custom_values": np.array([sp["custom"] for sp in SPEC], np.float64), "anchors_dtype": np.array(str(anchors.dtype))}

    # ---- TargetAssigner.assign, both modes, three frames
    rng = np.random.default_rng(97)
    frames = [draw_frame(rng, adict, (5, 4)), (np.zeros((0, 9), np.float32), []), draw_frame(rng, adict, (6, 0))]
    stored = {tag: dict(labels=[], targets=[]) for tag in assigners}
    for f, (gt, names) in enumerate(frames):
        gt_classes = np.array([CLASSES.index(n) + 1 for n in names], np.int32)
        out[f"gt_{f}"], out[f"gt_classes_{f}"] = gt, gt_classes
        for tag, asg in assigners.items():
            r = asg.assign(anchors, adict, gt, None, gt_classes=gt_classes, gt_names=np.array(names),
                           matched_thresholds=ret["matched_thresholds"], unmatched_thresholds=ret["unmatched_thresholds"])
            assert r["bbox_targets"].shape == (len(anchors), 9)
            if len(gt):
                assert r["bbox_targets"].dtype == np.float64, r["bbox_targets"].dtype
            stored[tag]["labels"].append(r["labels"]); stored[tag]["targets"].append(np.asarray(r["bbox_targets"], np.float64))
        print("frame", f, {tag: [int((stored[tag]["labels"][-1] == k).sum()) for k in (-1, 0, 1, 2)] for tag in assigners})
    for tag in assigners:
        lab, tg = np.stack(stored[tag]["labels"]), np.stack(stored[tag]["targets"])
        assert not tg[lab <= 0].any()
        pos = np.argwhere(lab > 0)
        out[f"labels_{tag}"] = lab.astype(np.int8)
        out[f"target_rows_{tag}"] = pos.astype(np.int32)                 # bbox_targets are zero outside the positives
        out[f"target_vals_{tag}"] = tg[pos[:, 0], pos[:, 1]]              # float64, as the reference returns them

    # ---- second_box_decode (torch) of random encodings against the anchors
    tg_ = torch.Generator().manual_seed(5)
    pick = torch.randperm(len(anchors), generator=tg_)[:64]
    enc = torch.randn(64, 9, generator=tg_, dtype=torch.float64) * 0.4
    dec = box_torch_ops.second_box_decode(enc, torch.from_numpy(anchors)[pick])
    out.update(decode_rows=pick.numpy().astype(np.int32), decode_enc=enc.numpy(), decode_out=dec.numpy())

    # ---- create_loss + get_direction_target in float64, nine non-uniform code weights
    # (on LOSS_ANCHORS anchors, to keep the file small: every anchor that is positive or don't-care in some frame, then background
    # ones; the inputs are float32 values widened, so that a float32 kernel reads exactly what the reference read)
    lab_all = out["labels_per_class"].astype(np.int32)
    reg_all = np.zeros((*lab_all.shape, 9))
    rows = out["target_rows_per_class"]
    reg_all[rows[:, 0], rows[:, 1]] = out["target_vals_per_class"]
    hot = np.nonzero((lab_all != 0).any(0))[0]
    cold = np.setdiff1d(np.arange(lab_all.shape[1]), hot)
    sel = np.sort(np.concatenate([hot, cold[:LOSS_ANCHORS - len(hot)]]))
    assert len(sel) == LOSS_ANCHORS and len(hot) < LOSS_ANCHORS
    lab_np, reg_np = lab_all[:, sel], reg_all[:, sel].astype(np.float32).astype(np.float64)
    b, n = lab_np.shape
    f32 = lambda t: t.float().double()
    cls = f32(torch.randn(b, n, 2, generator=tg_, dtype=torch.float64) * 2 - 2).requires_grad_()
    box = f32(torch.randn(b, n, 9, generator=tg_, dtype=torch.float64) * 0.3).requires_grad_()
    dirp = f32(torch.randn(b, n, 2, generator=tg_, dtype=torch.float64)).requires_grad_()
    imp = f32(torch.rand(b, n, generator=tg_, dtype=torch.float64) * 1.5 + 0.5)
    lab, reg = torch.from_numpy(lab_np), torch.from_numpy(reg_np)
    cls_w, reg_w, cared = V.prepare_loss_weights(lab, pos_cls_weight=LOSS["pos_cls_weight"], neg_cls_weight=LOSS["neg_cls_weight"],
                                                 loss_norm_type=V.LossNormType.NormByNumPositives, dtype=torch.float64)
    cls_t = (lab * cared.type_as(lab)).unsqueeze(-1)
    loc_ftor = losses.WeightedSmoothL1LocalizationLoss(sigma=LOSS["sigma"], code_weights=CODE_WEIGHTS, codewise=True)
    loc_ftor._code_weights = loc_ftor._code_weights.double()
    cls_ftor = losses.SigmoidFocalClassificationLoss(gamma=LOSS["gamma"], alpha=LOSS["alpha"])
    dir_ftor = losses.WeightedSoftmaxClassificationLoss()
    loc_loss, cls_loss = V.create_loss(loc_ftor, cls_ftor, box_preds=box, cls_preds=cls, cls_targets=cls_t, cls_weights=cls_w * imp,
                                       reg_targets=reg, reg_weights=reg_w * imp, num_class=2, encode_rad_error_by_sin=True,
                                       encode_background_as_zeros=True, box_code_size=9, sin_error_factor=LOSS["sin_error_factor"],
                                       num_direction_bins=2)
    loc_red = loc_loss.sum() / b * LOSS["localization_weight"]
    cls_red = cls_loss.sum() / b * LOSS["classification_weight"]
    pos_l, neg_l = V._get_pos_neg_loss(cls_loss, lab)
    anc_t = torch.from_numpy(a32[sel].astype(np.float64)).unsqueeze(0).repeat(b, 1, 1)
    dir_t = V.get_direction_target(anc_t, reg, dir_offset=LOSS["direction_offset"], num_bins=2)
    w = (lab > 0).type_as(dirp) * imp
    w = w / torch.clamp(w.sum(-1, keepdim=True), min=1.0)
    dir_loss = dir_ftor(dirp, dir_t, weights=w).sum() / b
    loss = loc_red + cls_red + dir_loss * LOSS["direction_loss_weight"]
    loss.backward()
    out.update(loss_anchor_rows=sel.astype(np.int32), loss_labels=lab_np.astype(np.int8), loss_reg=reg_np.astype(np.float32),
               loss_cls=cls.detach().numpy().astype(np.float32), loss_box=box.detach().numpy().astype(np.float32),
               loss_dir=dirp.detach().numpy().astype(np.float32), loss_importance=imp.numpy().astype(np.float32),
               loss_out6=np.array([loss.item(), cls_red.item(), loc_red.item(), dir_loss.item(),
                                   pos_l.item() / LOSS["pos_cls_weight"], neg_l.item() / LOSS["neg_cls_weight"]], np.float64),
               loss_d_cls=cls.grad.numpy(), loss_d_box=box.grad.numpy(), loss_d_dir=dirp.grad.numpy(),
               code_weights=np.array(CODE_WEIGHTS, np.float64), loss_cfg=np.array([LOSS[k] for k in sorted(LOSS)], np.float64),
               loss_cfg_keys=np.array(sorted(LOSS)))
    print("loss", loss.item(), "loc", loc_red.item(), "cls", cls_red.item(), "dir", dir_loss.item(), "pos", pos_l.item(), "neg", neg_l.item())

    # ---- random_flip / global_rotation_v2 / global_scaling_v2 on [G, 9] boxes: all four flip combinations, fixed angle and scale
    aug_gt = np.concatenate([frames[0][0], frames[2][0]])
    out["aug_boxes"] = aug_gt
    real_choice, real_uniform = np.random.choice, np.random.uniform
    try:
        for fx in (0, 1):
            for fy in (0, 1):
                draws = iter([bool(fx), bool(fy)])
                np.random.choice = lambda *a, **k: next(draws)
                g, pts = aug_gt.copy(), np.zeros((1, 4), np.float32)
                g, pts = preprocess.random_flip(g, pts, 0.5, True, True)
                out[f"aug_flip_{fx}{fy}"] = g.copy()
                np.random.uniform = lambda *a, **k: ANGLE
                g, pts = preprocess.global_rotation_v2(g, pts, -1.0, 1.0)
                np.random.uniform = lambda *a, **k: SCALE
                g, pts = preprocess.global_scaling_v2(g, pts, 0.9, 1.1)
                assert g.dtype == np.float32 and g.shape[1] == 9
                out[f"aug_full_{fx}{fy}"] = g.copy()
    finally:
        np.random.choice, np.random.uniform = real_choice, real_uniform
    out["aug_angle"], out["aug_scale"] = np.float64(ANGLE), np.float64(SCALE)
    path = os.path.join(HERE, "box_custom.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
