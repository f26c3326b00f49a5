"""References and comparisons for boxes with custom values (rows of box_ndim = 7 + custom_ndim values; nuScenes velocity: 9).

  fixture / fixture_targets        tests/golden/box_custom.npz, produced by executing the reference (make_golden_box_custom.py)
  encode_ref / decode_ref          GroundBox3dCoder with custom_ndim in float64: train_ref_helpers.box_encode / predict_ref_helpers.
                                   decode_reference64 on columns 0-6, column 7 + j = g - a / t + a
  assign_ref_nd                    train_ref_helpers.assign_ref per anchor range, with the matched box's custom residuals
  loss_nd                          VoxelNet.loss on rows of box_ndim values under autograd, in any precision: the float64 yardstick of
                                   sec_second_loss_nd_f32, and (float32, with a planted ``mistake``) what the host tests run through
                                   the same comparisons
  velocity_ref                     the reference's shape[1] == 9 branches of random_flip / global_rotation_v2 / global_scaling_v2
  check_*                          the comparisons tests/test_gpu_box_custom.py applies to the kernels; tests/test_box_custom_host.py
                                   applies them to float32 emulations, correct ones and ones with a planted mistake

Built on train_ref_helpers, predict_ref_helpers and augment_helpers by import."""
import os

import numpy as np
import torch

import augment_helpers as A
import predict_ref_helpers as P
import train_ref_helpers as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_custom.npz")
BOX_MAX_NDIM = 11
VELOCITY_TOL = 16 * 2.0 ** -24          # x (|vx| + |vy| + 1): the constant README states for the augmentation kernel's values


def fixture():
    return dict(np.load(GOLDEN))


def fixture_cfg(g):
    """The second_amd config entries of the fixture's two anchor generators."""
    return dict(anchor_sizes=[[1.6, 3.9, 1.56], [0.6, 0.8, 1.73]], rotations=[0, 1.57], group_rotations={1: [0]},
                anchor_ranges=[[-4.0, -4.8, -1.0, 4.0, 4.8, -1.0], [-4.0, -4.8, -0.6, 4.0, 4.8, -0.6]],
                anchor_custom_values=[list(v) for v in g["custom_values"]])


def fixture_targets(g, tag):
    """labels int32 [F, A] and bbox_targets float64 [F, A, 9] of mode ``tag`` ("per_class" / "all"; stored sparsely)."""
    lab = g[f"labels_{tag}"].astype(np.int32)
    tg = np.zeros((*lab.shape, g["anchors"].shape[1]))
    rows = g[f"target_rows_{tag}"]
    tg[rows[:, 0], rows[:, 1]] = g[f"target_vals_{tag}"]
    return lab, tg


def fixture_frames(g):
    return [(g[f"gt_{f}"], g[f"gt_classes_{f}"]) for f in range(g["labels_per_class"].shape[0])]


# ------------------------------------------------------------------------------------------------------------ encode / decode
def encode_ref(gt, anchors):
    """second_box_encode with custom values (box_np_ops.py:47-81) in float64: [N, nd] x [N, nd] -> [N, nd]."""
    g, a = np.asarray(gt, np.float64), np.asarray(anchors, np.float64)
    return np.concatenate([T.box_encode(g[:, :7], a[:, :7]), g[:, 7:] - a[:, 7:]], 1)


def decode_ref(enc, anchors):
    """second_box_decode with custom values (box_torch_ops.py:64-102) in float64 on torch tensors [..., nd]."""
    return torch.cat([P.decode_reference64(enc[..., :7], anchors[..., :7]), enc[..., 7:].double() + anchors[..., 7:].double()], -1)


def exact_sum_values(rng, shape):
    """float32 values of either sign with magnitudes in [2^-10, 64]: the float64 sum of two of them is exact (24-bit significands whose
    exponents differ by at most 16), so float32(float64(e) + float64(a)) is the correctly rounded float32 sum."""
    v = (2.0 ** rng.uniform(-10, 6, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    assert np.all((np.abs(v) >= 2.0 ** -10) & (np.abs(v) <= 64))
    return v


def check_decode_custom(got, enc, anc):
    """Custom columns of a decode, bit for bit: got [..., c] float32 against float32(float64(e) + float64(a))."""
    want = (np.asarray(enc, np.float64) + np.asarray(anc, np.float64)).astype(np.float32)
    assert P.same_bits_f32(got, want), "custom columns of the decode"


# ------------------------------------------------------------------------------------------------------------------ assignment
def assign_ref_nd(anchors, gt, gt_classes, begins, class_ids, matched, unmatched, mask=None):
    """train_ref_helpers.assign_per_class_ref on rows of nd values: -> labels int32 [A], targets float64 [A, nd], arg [A] (index of the
    matched box in ``gt`` for labels > 0, -1 otherwise).  The matching sees columns 0-6."""
    anchors, gt = np.asarray(anchors, np.float64), np.asarray(gt, np.float64).reshape(-1, np.asarray(anchors).shape[1])
    gt_classes = np.asarray(gt_classes, np.int32)
    n, nd = anchors.shape
    a7, g7 = anchors[:, :7], gt[:, :7]
    labels = T.assign_per_class_ref(a7, g7, gt_classes, begins, class_ids, matched, unmatched, mask=mask)[0]
    arg = np.full(n, -1)
    keep = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    gmax_all = None
    if len(gt) and any(k == 0 for k in class_ids):
        live = np.zeros(n, bool)
        for c, k in enumerate(class_ids):
            if k == 0:
                live[begins[c]:begins[c + 1]] = True
        ov = T.iou_eps0(T.near_boxes(a7[live & keep]), T.near_boxes(g7))
        gmax_all = ov.max(0) if len(ov) else np.zeros(len(gt))
    for c, k in enumerate(class_ids):
        s = slice(begins[c], begins[c + 1])
        if begins[c] == begins[c + 1] or len(gt) == 0:
            continue
        sel = np.ones(len(gt), bool) if k == 0 else gt_classes == k
        if not sel.any():
            continue
        info = T.assign_ref(a7[s], g7[sel], matched[c], unmatched[c], gt_classes[sel], None, None if mask is None else keep[s],
                            gmax=gmax_all if k == 0 else None)[3]
        arg[s] = np.where(info["arg"] >= 0, np.nonzero(sel)[0][np.maximum(info["arg"], 0)], -1)
    arg[labels <= 0] = -1
    targets = np.zeros((n, nd))
    fg = labels > 0
    targets[fg] = encode_ref(gt[arg[fg]], anchors[fg])
    return labels, targets, arg


def matched_rows(anchors, gt, targets7, labels, candidates):
    """The ground-truth row every positive anchor of one frame was encoded against, read off the kernel's own 7-column targets:
    the FIRST candidate k with float32(g_k[6] - a[6]) == t[6] and float32((g_k[2] - a[2]) / a[5]) == t[2] (IEEE operations, the ones
    the kernel performs).  ``candidates`` [A, G] bool: the boxes the anchor's range is matched against.  Every further candidate that
    reproduces the two values must be a duplicate of the first in all seven columns (asserted): then "first" is the matching's own
    rule (first index on ties)."""
    a, g = np.asarray(anchors, np.float32), np.asarray(gt, np.float32)
    arg = np.full(len(a), -1)
    for i in np.nonzero(np.asarray(labels) > 0)[0]:
        t6 = g[:, 6] - a[i, 6]
        t2 = (g[:, 2] - a[i, 2]) / a[i, 5]
        hit = np.nonzero(candidates[i] & (t6 == targets7[i, 6]) & (t2 == targets7[i, 2]))[0]
        assert len(hit), f"anchor {i}: no ground truth reproduces its targets"
        assert np.all(g[hit, :7] == g[hit[0], :7]), f"anchor {i}: distinct boxes reproduce its targets"
        arg[i] = hit[0]
    return arg


def check_assign_custom(got, anchors, gt, arg):
    """Custom target columns of one frame, bit for bit: got [A, c] float32 = float32(g - a) where arg >= 0, +0.0 elsewhere."""
    a, g = np.asarray(anchors, np.float32)[:, 7:], np.asarray(gt, np.float32).reshape(-1, np.asarray(anchors).shape[1])[:, 7:]
    want = np.zeros_like(a)
    fg = arg >= 0
    want[fg] = (g[arg[fg]].astype(np.float64) - a[fg].astype(np.float64)).astype(np.float32)
    assert P.same_bits_f32(got, want), "custom target columns"


# ------------------------------------------------------------------------------------------------------------------------ loss
def loss_nd(cls, box, dirp, labels, reg, anchors, importance, num_class, num_direction_bins, dtype=torch.float64, mistake=None, **cfg):
    """VoxelNet.loss (voxelnet.py:239-312: prepare_loss_weights, create_loss with add_sin_difference, get_direction_target, the three
    loss functors of core/losses.py) on box rows of nd values, on ``dtype`` tensors under autograd.  -> (out6, d_cls, d_box, d_dir) as
    numpy arrays, out6 = (loss, cls_loss_reduced, loc_loss_reduced, dir_loss_reduced, cls_pos_loss, cls_neg_loss).  ``cfg``: entries
    of train_ref_helpers.LOSS_DEFAULTS, with code_weights of nd values.
    ``mistake`` plants one: "sin_last" (sin-difference on the last column), "weight_shift" (code weight j on column j - 1),
    "dir_last" (direction target from column nd - 1)."""
    p = dict(T.LOSS_DEFAULTS, **cfg)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    labels = torch.from_numpy(np.ascontiguousarray(labels)).long()
    b, n = labels.shape
    nd = np.asarray(box).shape[-1]
    assert len(p["code_weights"]) == nd
    cls, box = t(cls).reshape(b, n, num_class).requires_grad_(), t(box).reshape(b, n, nd).requires_grad_()
    leaves = [cls, box]
    reg, anchors, imp = t(reg), t(anchors), t(importance)
    pos, neg = (labels > 0).to(dtype), (labels == 0).to(dtype)
    norm = pos.sum(1, keepdim=True).clamp(min=1.0)
    # classification: sigmoid focal loss on one-hot targets, background encoded as zeros
    wcls = (neg * p["neg_cls_weight"] + pos * p["pos_cls_weight"]) / norm * imp
    tgt = torch.nn.functional.one_hot(labels.clamp(min=0), num_class + 1)[..., 1:].to(dtype)
    ce = cls.clamp(min=0) - cls * tgt + torch.log1p(torch.exp(-cls.abs()))
    prob = torch.sigmoid(cls)
    pt = tgt * prob + (1 - tgt) * (1 - prob)
    mod = torch.pow(1 - pt, p["gamma"]) if p["gamma"] else torch.ones_like(pt)
    at = tgt * p["alpha"] + (1 - tgt) * (1 - p["alpha"])
    cls_loss = mod * at * ce * wcls.unsqueeze(-1)
    # localisation: smooth L1 on the sin-difference encoding of the rotation column
    sc = nd - 1 if mistake == "sin_last" else 6
    k = p["sin_error_factor"]
    pr, tr = k * box[..., sc:sc + 1], k * reg[..., sc:sc + 1]
    bp = torch.cat([box[..., :sc], torch.sin(pr) * torch.cos(tr), box[..., sc + 1:]], -1)
    rt_ = torch.cat([reg[..., :sc], torch.cos(pr) * torch.sin(tr), reg[..., sc + 1:]], -1)
    cw = torch.tensor(p["code_weights"], dtype=dtype)
    if mistake == "weight_shift":
        cw = torch.cat([cw[1:], cw[:1]])
    diff = cw * (bp - rt_)
    ad, s2 = diff.abs(), p["sigma"] ** 2
    loc_loss = torch.where(ad <= 1.0 / s2, 0.5 * s2 * ad * ad, ad - 0.5 / s2) * (pos / norm * imp).unsqueeze(-1)
    cls_red = cls_loss.sum() / b * p["classification_weight"]
    loc_red = loc_loss.sum() / b * p["localization_weight"]
    if num_class == 1:
        cls_pos, cls_neg = (cls_loss.squeeze(-1) * pos).sum() / b, (cls_loss.squeeze(-1) * neg).sum() / b
    else:
        cls_pos, cls_neg = cls_loss[..., 1:].sum() / b, cls_loss[..., 0].sum() / b
    loss = loc_red + cls_red
    dir_red = torch.zeros((), dtype=dtype)
    bins = int(num_direction_bins)
    if bins > 0:
        dirp = t(dirp).reshape(b, n, bins).requires_grad_()
        leaves.append(dirp)
        dc = nd - 1 if mistake == "dir_last" else 6
        rot = reg[..., dc] + anchors[None, :, dc] - p["direction_offset"]
        off = rot - torch.floor(rot / (2 * np.pi)) * (2 * np.pi)
        tbin = torch.floor(off / (2 * np.pi / bins)).long().clamp(0, bins - 1)
        w = pos * imp
        w = w / w.sum(1, keepdim=True).clamp(min=1.0)
        nll = torch.logsumexp(dirp, -1) - torch.gather(dirp, -1, tbin.unsqueeze(-1)).squeeze(-1)
        dir_red = (nll * w).sum() / b
        loss = loss + dir_red * p["direction_loss_weight"]
    grads = torch.autograd.grad(loss, leaves)
    out6 = torch.stack([loss, cls_red, loc_red, dir_red, cls_pos / p["pos_cls_weight"], cls_neg / p["neg_cls_weight"]]).detach().numpy()
    g = [x.numpy() for x in grads]
    return out6, g[0], g[1], (g[2] if bins > 0 else None)


def check_loss(got, want):
    """The comparison of tests/test_gpu_train_edges.py (_check_scalars, _check_grad): out6 within rtol 1e-4 (a term whose reference is
    exactly zero within 1e-7), every gradient within rtol 1e-4 plus 1e-6 of the tensor's largest reference magnitude."""
    g6, w6 = np.asarray(got[0], np.float64), np.asarray(want[0], np.float64)
    tol = np.where(w6 == 0, 1e-7, 1e-4 * np.abs(w6))
    assert np.all(np.abs(g6 - w6) <= tol), (g6, w6)
    for name, g, w in zip(("d_cls", "d_box", "d_dir"), got[1:], want[1:]):
        assert (g is None) == (w is None), name
        if w is not None:
            np.testing.assert_allclose(np.asarray(g, np.float64), w, rtol=1e-4, atol=1e-6 * np.abs(w).max() + 1e-9, err_msg=name)


def loss_case_nd(seed, batch, n_anchor, num_class, bins, nd, direction_offset=0.0, **kw):
    """train_ref_helpers.loss_case widened to nd columns: custom predictions, targets and anchor values of the scale of a velocity."""
    c = T.loss_case(seed, batch, n_anchor, num_class, bins, direction_offset=direction_offset, **kw)
    rng = np.random.default_rng(seed + 1000)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    c["box"] = np.concatenate([c["box"], f(batch, n_anchor, nd - 7) * 0.7], -1)
    c["reg"] = np.concatenate([c["reg"], f(batch, n_anchor, nd - 7) * 1.5], -1)
    c["anchors"] = np.concatenate([c["anchors"], f(n_anchor, nd - 7)], -1)
    return c


# -------------------------------------------------------------------------------------------------------------------- velocity
def velocity_ref(v, flip_x, flip_y, angle, scale, dtype=np.float64, rotate=True, mistake=None):
    """Columns 7, 8 of [G, 9] boxes through random_flip (y then x), global_rotation_v2 and global_scaling_v2 (preprocess.py:749-799):
    (vx, vy) @ [[c, -s], [s, c]] = (vx c + vy s, -vx s + vy c), then both times the scale.  ``rotate`` False: the flips only.
    ``mistake``: "rot_sign" (+angle), "flip_col" (y flip negates column 7), "no_scale", "translate" (a translation added)."""
    v = np.array(v, dtype)
    vx, vy = v[:, 0].copy(), v[:, 1].copy()
    if flip_y:
        if mistake == "flip_col":
            vx = -vx
        else:
            vy = -vy
    if flip_x:
        vx = -vx
    if rotate:
        ang = dtype(-angle if mistake == "rot_sign" else angle)
        c, s = np.cos(ang), np.sin(ang)
        vx, vy = vx * c + vy * s, vy * c - vx * s
        if mistake != "no_scale":
            vx, vy = vx * dtype(scale), vy * dtype(scale)
        if mistake == "translate":
            vx, vy = vx + dtype(0.5), vy + dtype(-0.25)
    return np.stack([vx, vy], 1)


def check_velocity(got, v_in, want):
    """|got - want| <= 16 * 2^-24 * (|vx| + |vy| + 1) per row, (vx, vy) the row's input velocity."""
    got, want, v_in = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(v_in, np.float64)
    bound = VELOCITY_TOL * (np.abs(v_in).sum(1, keepdims=True) + 1.0)
    err = np.abs(got - want)
    assert np.all(err <= bound), f"velocity off by {(err / bound).max():.2f} x the bound"


def velocity_batch(seed, box_counts, nd=9):
    """A batch of augment_helpers.build_frame frames (boxes spread over the range, some invalid) widened to nd columns with
    velocities from N(0, 3), and frame parameters that flip / rotate / scale / translate every frame differently.
    -> dict(boxes [G, nd], box_offsets, valid, classes, importance, loc_transform [G, 3], rot_transform [G], params [B, 8]), float32."""
    frames = [A.build_frame(seed + 17 * f, n, 1, 1, "invalid" if n >= 5 else "") for f, n in enumerate(box_counts)]
    batch = A.concat_frames(frames)
    rng = np.random.default_rng(seed)
    g = len(batch["boxes"])
    out = {k: batch[k] for k in ("box_offsets", "valid", "classes", "importance")}
    out["boxes"] = np.concatenate([batch["boxes"], rng.normal(0, 3, (g, nd - 7)).astype(np.float32)], 1)
    out["loc_transform"] = rng.normal(0, 0.3, (g, 3)).astype(np.float32)
    out["rot_transform"] = rng.uniform(-0.3, 0.3, g).astype(np.float32)
    b = len(box_counts)
    params = np.zeros((b, 8), np.float32)
    params[:, 0], params[:, 1] = np.arange(b) % 2, (np.arange(b) // 2) % 2           # every flip combination within four frames
    params[:, 2] = rng.uniform(-np.pi / 4, np.pi / 4, b)
    params[:, 3] = rng.uniform(0.95, 1.05, b)
    params[:, 4:7] = rng.normal(0, 0.2, (b, 3))
    out["params"] = params
    return out


# ---------------------------------------------------------------------------------------------------- whole path, reduced geometry
CAR_RANGE = [0, -5.6, -3, 14.4, 5.6, 1]          # the 28 x 36 feature map of tests/test_gpu_train_step_audit.py


def car_velo_cfg(custom=(0.0, 0.0)):
    """car.fhd on the reduced range with ``anchor_custom_values``: box rows of 7 + len(custom) values."""
    from second_amd.models import CAR_FHD
    x0, y0, _, x1, y1, _ = CAR_RANGE
    return dict(CAR_FHD, name="car.fhd.velo", point_cloud_range=list(CAR_RANGE), anchor_ranges=[[x0, y0, -1.0, x1, y1, -1.0]],
                post_center_range=[x0, y0, -2.2, x1, y1, 0.8], max_voxels=8000, anchor_custom_values=list(custom))


def car_clouds(seeds, voxels=2600):
    from second_amd import synthetic as syn
    return [syn.syn_kitti_cloud(s, num_points=voxels + 400 + 37 * i, num_voxels=voxels + 91 * i,
                                point_cloud_range=tuple(float(v) for v in CAR_RANGE)) for i, s in enumerate(seeds)]


def trained_like_on_device(det, calib_cloud):
    """Seeded weights that behave like a trained detector's (synthetic.randomise_like_trained / sharpen_heads: distinct scores, empty
    regions below the threshold), the heads calibrated through the fp32 device forward as bench.py does.  ``det`` on the CPU, in
    eval mode; returns it on the device."""
    from second_amd import synthetic as syn
    syn.randomise_like_trained(det, seed=1)
    det = det.eval().cuda()
    pts, offs = syn.batch_clouds([calib_cloud])
    with torch.no_grad():
        vox = det.voxel_generator.generate_device(torch.from_numpy(pts).cuda(), torch.from_numpy(offs).cuda(), mean_features=4)
        preds = det.network_forward(vox["mean"], vox["coordinates"], 1)
        syn.sharpen_heads(det, preds["cls_preds"].float(), preds["box_preds"].float())
    return det


def standin_net(cfg, custom_ndim=2, **coder_kw):
    """tests/reference_standin.py's VoxelNet for ``cfg`` with the attributes of a reference network whose box coder is
    GroundBox3dCoder(custom_ndim=...) and whose anchor generators carry custom_values (what dropin.model_config reads)."""
    import types
    from reference_standin import build_voxelnet
    net = build_voxelnet(cfg)
    coder = types.SimpleNamespace(code_size=7 + custom_ndim + (1 if coder_kw.get("vec_encode") else 0), custom_ndim=custom_ndim,
                                  vec_encode=False, linear_dim=False)
    coder.__dict__.update(coder_kw)
    net._box_coder = net.target_assigner.box_coder = coder
    net.target_assigner._anchor_generators = [types.SimpleNamespace(_custom_values=[0.0] * custom_ndim, class_name="Car")]
    return net
