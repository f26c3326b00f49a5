"""float64 references of the training-side kernels (csrc/train.hip), written from the formulas the kernels' comments state:

  assign_ref / assign_per_class_ref   anchor <-> ground-truth matching + box encoding of one frame (k_assign_max, k_assign_write)
  lattice_case                        anchors and ground truth on a 1/8 m lattice where fp32 and fp64 agree on EVERY comparison
  loss_case / loss_ref                tests/reference_standin.py::standin_loss on float64 tensors under autograd
  adamw_ref                           the formula in the comment above k_flat_sumsq

tests/test_train_ref_host.py pins them to the fixtures the reference itself produced; tests/test_gpu_train_edges.py compares the
kernels with them."""
import types

import numpy as np
import torch

from reference_standin import standin_loss, _named

LOSS_KEYS = ("alpha", "gamma", "sigma", "pos_cls_weight", "neg_cls_weight", "classification_weight", "localization_weight",
             "direction_loss_weight", "direction_offset", "sin_error_factor", "code_weights")
# car.fhd values; tests/test_train_ref_host.py checks that they are second_amd.ops.LOSS_DEFAULTS
LOSS_DEFAULTS = dict(alpha=0.25, gamma=2.0, sigma=3.0, pos_cls_weight=1.0, neg_cls_weight=1.0, classification_weight=1.0,
                     localization_weight=2.0, direction_loss_weight=0.2, direction_offset=0.0, sin_error_factor=1.0,
                     code_weights=(1.0,) * 7)
# every hyper-parameter off its default, focal gamma on the powf branch
LOSS_NONDEFAULT = dict(gamma=1.5, alpha=0.4, sigma=2.0, pos_cls_weight=2.0, neg_cls_weight=0.5, classification_weight=1.5,
                       localization_weight=0.7, direction_loss_weight=0.3, direction_offset=0.78, sin_error_factor=2.0,
                       code_weights=(1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 2.0))


# ------------------------------------------------------------------------------------------------------------- target assignment
def near_boxes(boxes, dtype=np.float64):
    """[N, 7] (x, y, z, w, l, h, r) -> [N, 4] axis-aligned (x0, y0, x1, y1) of the nearer of the standing / lying orientation:
    the rotation is reduced to [-pi/2, pi/2) and the box lies (w and l swap) when its magnitude exceeds pi/4."""
    b = np.asarray(boxes, dtype)
    pi = dtype(np.pi)
    r = b[:, 6]
    a = np.abs(r - np.floor(r / pi + dtype(0.5)) * pi)
    swap = a > pi / dtype(4)
    dx, dy = np.where(swap, b[:, 4], b[:, 3]), np.where(swap, b[:, 3], b[:, 4])
    return np.stack([b[:, 0] - dx / 2, b[:, 1] - dy / 2, b[:, 0] + dx / 2, b[:, 1] + dy / 2], 1)


def swap_margin(boxes):
    """Distance of the reduced rotation's magnitude from the pi/4 swap boundary of near_boxes (float64)."""
    r = np.asarray(boxes, np.float64)[:, 6]
    return np.abs(np.abs(r - np.floor(r / np.pi + 0.5) * np.pi) - np.pi / 4)


def iou_eps0(a, q):
    """[N, 4] x [K, 4] -> [N, K] intersection over union with eps 0 (widths are plain differences); no overlap gives 0."""
    iw = np.minimum(a[:, None, 2], q[None, :, 2]) - np.maximum(a[:, None, 0], q[None, :, 0])
    ih = np.minimum(a[:, None, 3], q[None, :, 3]) - np.maximum(a[:, None, 1], q[None, :, 1])
    inter = iw * ih
    area_a = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None]
    area_q = ((q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1]))[None, :]
    ok = (iw > 0) & (ih > 0)
    return np.where(ok, inter / np.where(ok, area_a + area_q - inter, 1), 0)


def box_encode(gt, anchors):
    """Residuals of matched ground truth against anchors, both [N, 7]: centre offsets over the anchor's BEV diagonal (z over its
    height), log size ratios, rotation difference."""
    g, a = np.asarray(gt, np.float64), np.asarray(anchors, np.float64)
    diag = np.sqrt(a[:, 4] ** 2 + a[:, 3] ** 2)
    return np.stack([(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / a[:, 5], np.log(g[:, 3] / a[:, 3]),
                     np.log(g[:, 4] / a[:, 4]), np.log(g[:, 5] / a[:, 5]), g[:, 6] - a[:, 6]], 1)


def _match(ov, gmax, matched, unmatched, classes):
    """Labels of the anchors whose overlaps are the rows of ``ov``, given every ground truth's best overlap ``gmax``."""
    arg = ov.argmax(1)                                        # first index on ties
    mx = ov[np.arange(len(ov)), arg]
    gmax = np.where(gmax == 0, -1.0, gmax)                    # a ground truth nothing overlaps forces nobody
    force = (ov == gmax[None, :]).any(1)
    pos = mx >= matched
    labels = np.full(len(ov), -1, np.int32)
    labels[mx < unmatched] = 0
    labels[force | pos] = classes[arg[force | pos]]           # forced anchors take the class of their OWN argmax, also after the
    return labels, arg, mx, pos, force                        # background pass


def assign_ref(anchors, gt, matched, unmatched, gt_classes=None, gt_importance=None, mask=None, gmax=None, importance_table=None):
    """One frame.  anchors [A, 7], gt [G, 7]; ``matched`` / ``unmatched`` scalars or per-anchor arrays.  -> labels int32 [A],
    targets float64 [A, 7], importance float32 [A], and a dict with max / argmax / positive / forced per anchor.
    ``gmax``: the ground truths' best overlaps where they are taken over more anchors than these (assign_all over several ranges).
    ``importance_table``: the array positives index with their argmax (default: gt_importance)."""
    anchors, gt = np.asarray(anchors, np.float64), np.asarray(gt, np.float64).reshape(-1, 7)
    n = len(anchors)
    keep = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    labels, targets, imp = np.full(n, -1, np.int32), np.zeros((n, 7)), np.where(keep, 1.0, 0.0).astype(np.float32)
    info = dict(max=np.full(n, -1.0), arg=np.full(n, -1), pos=np.zeros(n, bool), force=np.zeros(n, bool))
    if len(gt) == 0:
        labels[keep] = 0
        return labels, targets, imp, info
    classes = np.ones(len(gt), np.int32) if gt_classes is None else np.asarray(gt_classes, np.int32)
    table = importance_table if importance_table is not None else gt_importance
    ov = iou_eps0(near_boxes(anchors[keep]), near_boxes(gt))
    if gmax is None:
        gmax = ov.max(0) if len(ov) else np.zeros(len(gt))
    lab, arg, mx, pos, force = _match(ov, gmax, np.broadcast_to(matched, (n,))[keep], np.broadcast_to(unmatched, (n,))[keep], classes)
    idx = np.nonzero(keep)[0]
    labels[idx] = lab
    if table is not None:
        imp[idx[pos]] = np.asarray(table, np.float32)[arg[pos]]            # only anchors at or above `matched`, not the forced ones
    fg = lab > 0
    targets[idx[fg]] = box_encode(gt[arg[fg]], anchors[idx[fg]])
    for k, v in (("max", mx), ("arg", arg), ("pos", pos), ("force", force)):
        info[k][idx] = v
    return labels, targets, imp, info


def assign_per_class_ref(anchors, gt, gt_classes, begins, class_ids, matched, unmatched, gt_importance=None, mask=None):
    """One frame over anchor ranges [begins[c], begins[c + 1]).  class_ids[c] = k > 0: the range is matched against the boxes of
    class k only; a positive's importance is the FRAME's importance array read at the box's position WITHIN the class's boxes.
    class_ids[c] = 0: every box, the range's own thresholds, a ground truth's best overlap taken over the anchors of all ranges."""
    anchors, gt = np.asarray(anchors, np.float64), np.asarray(gt, np.float64).reshape(-1, 7)
    gt_classes = np.asarray(gt_classes, np.int32)
    n = len(anchors)
    labels, targets, imp = np.full(n, -1, np.int32), np.zeros((n, 7)), np.ones(n, np.float32)
    keep = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    gmax_all = None
    if len(gt) and any(k == 0 for k in class_ids):
        live = np.zeros(n, bool)
        for c, k in enumerate(class_ids):
            if k == 0:
                live[begins[c]:begins[c + 1]] = True
        ov = iou_eps0(near_boxes(anchors[live & keep]), near_boxes(gt))
        gmax_all = ov.max(0) if len(ov) else np.zeros(len(gt))
    for c, k in enumerate(class_ids):
        s = slice(begins[c], begins[c + 1])
        if begins[c] == begins[c + 1]:
            continue
        m = None if mask is None else keep[s]
        if k == 0:
            l, t, i, _ = assign_ref(anchors[s], gt, matched[c], unmatched[c], gt_classes, gt_importance, m, gmax=gmax_all)
        else:
            sel = gt_classes == k
            l, t, i, _ = assign_ref(anchors[s], gt[sel], matched[c], unmatched[c], gt_classes[sel], gt_importance, m)
        labels[s], targets[s], imp[s] = l, t, i
    return labels, targets, imp


def make_anchors(h, w, stride=1.0, size=(1.5, 4.0, 1.5), z=-1.0, rotations=(0.0, np.pi / 2)):
    """[h * w * len(rotations), 7] float32 anchors centred on a lattice around the origin, index (y * w + x) * R + r."""
    ys = (np.arange(h) - (h - 1) // 2) * stride
    xs = (np.arange(w) - (w - 1) // 2) * stride
    out = np.zeros((h, w, len(rotations), 7))
    out[..., 0], out[..., 1], out[..., 2] = xs[None, :, None], ys[:, None, None], z
    out[..., 3:6] = size
    out[..., 6] = np.asarray(rotations)[None, None, :]
    return out.reshape(-1, 7).astype(np.float32)


def _lattice_frame(rng, anchors, n, dense):
    """n ground-truth boxes on the 1/8 m lattice (sizes in steps of 1/4 m, so corners stay on the 1/8 m lattice): boxes that sit
    tightly on an anchor, loosely on one, small ones (best overlap far below any threshold), duplicates of earlier boxes and boxes
    far outside the anchor map.  Only anchors among ``dense`` attract boxes, the rest stay background."""
    boxes = np.zeros((n, 7))
    for i in range(n):
        kind = rng.choice(5, p=[0.30, 0.38, 0.2, 0.06, 0.06]) if i >= 4 else 0
        a = anchors[rng.choice(dense)].astype(np.float64)
        if kind == 3 and i > 8:                               # duplicate (ties in the argmax: the first one wins)
            boxes[i] = boxes[rng.integers(0, i)]
            continue
        if kind == 4:                                         # overlaps no anchor at all
            boxes[i] = [40.0 + rng.integers(0, 160) / 8, -30.0 + rng.integers(0, 480) / 8, -1.0, 1.5, 4.0, 1.5, rng.uniform(-3, 3)]
        else:
            reach = (2, 2) if kind == 0 else (10, 14)
            lying = abs(a[6]) > 0.1
            off = np.array([rng.integers(-reach[0], reach[0] + 1), rng.integers(-reach[1], reach[1] + 1)]) / 8
            if lying:
                off = off[::-1]
            wl = (rng.integers(5, 9) / 4, rng.integers(14, 19) / 4) if kind != 2 else (rng.integers(2, 4) / 4, rng.integers(3, 6) / 4)
            rot = a[6] + rng.choice([0.0, np.pi, -np.pi, 0.0]) + rng.uniform(-0.7, 0.7)
            boxes[i] = [a[0] + off[0], a[1] + off[1], -1.0 + rng.integers(-4, 5) / 8, wl[0], wl[1], rng.integers(5, 8) / 4, rot]
        if swap_margin(boxes[i:i + 1])[0] < 2e-3:
            boxes[i, 6] += 0.01
    return boxes.astype(np.float32)


def lattice_stats(anchors, gt, matched, unmatched):
    """Group sizes of the plain (one class) assignment of one frame."""
    labels, _, _, info = assign_ref(anchors, gt, matched, unmatched)
    ov = iou_eps0(near_boxes(anchors), near_boxes(gt))
    mx = info["max"]
    ties = int(((ov == mx[:, None]) & (mx[:, None] > 0)).sum(1).__gt__(1).sum())
    g64 = np.asarray(gt, np.float64)
    dup = sum(1 for i in range(len(g64)) if (g64[:i] == g64[i]).all(1).any())
    return dict(pos_thr=int(info["pos"].sum()), forced_only=int((info["force"] & ~info["pos"]).sum()),
                forced_below_unmatched=int((info["force"] & (mx < unmatched)).sum()), background=int((labels == 0).sum()),
                dont_care=int((labels == -1).sum()), argmax_ties=ties, gt_no_overlap=int((ov.max(0) == 0).sum()), gt_duplicates=dup,
                on_threshold=int(((ov == matched) | (ov == unmatched)).sum()))


def assert_lattice_exact(anchors, gt, thresholds):
    """fp32 and fp64 agree bit for bit on every comparison the assignment of this frame makes."""
    for b in (anchors, gt):
        b64 = np.asarray(b, np.float64)
        assert np.all(b64[:, [0, 1, 3, 4]] * 8 == np.round(b64[:, [0, 1, 3, 4]] * 8)) and np.all(np.abs(b64[:, [0, 1, 3, 4]]) <= 64)
        assert np.all(swap_margin(b64) >= 1e-3), "rotation too close to the swap boundary of the near box"
        assert np.array_equal(near_boxes(b, np.float32).astype(np.float64), near_boxes(b, np.float64))
    if len(gt) == 0:
        return
    ov64 = iou_eps0(near_boxes(anchors), near_boxes(gt))
    ov32 = iou_eps0(near_boxes(anchors, np.float32), near_boxes(gt, np.float32))
    assert ov32.dtype == np.float32
    vals = np.unique(ov64[ov64 > 0])
    if len(vals) > 1:
        assert np.diff(vals).min() > 2.0 ** -22, np.diff(vals).min()
    assert len(np.unique(ov32[ov32 > 0])) == len(vals)              # distinct stays distinct, equal stays equal
    assert np.array_equal(ov32 > 0, ov64 > 0)
    for pair in thresholds:
        for t in pair:
            d = np.abs(ov64 - t)
            assert np.all((d == 0) | (d > 1e-6)), t
            assert np.array_equal(ov32 >= np.float32(t), ov64 >= t) and np.array_equal(ov32 < np.float32(t), ov64 < t), t
    # order: the rank of every overlap among the frame's distinct values is the same in both precisions
    assert np.array_equal(np.searchsorted(np.unique(ov32), ov32), np.searchsorted(np.unique(ov64), ov64))


LATTICE_THRESHOLDS = ((0.5, 0.375), (0.6, 0.45))
LATTICE_COUNTS = (300, 256, 257, 0, 1)


def lattice_case(seed, fm=(23, 19), counts=LATTICE_COUNTS, thresholds=LATTICE_THRESHOLDS):
    """Anchors of an fm[0] x fm[1] map with two rotations and one ground-truth frame per entry of ``counts``, with classes in
    {1, 2, 3} and importance per box.  Asserts (never filters) what makes the fp32 kernel and the fp64 reference comparable bit
    for bit, and that the largest frame holds every kind of anchor and ground truth the matching distinguishes.
    Frame 0 holds fewer than ten boxes of class 2 (some beyond index 256 when it is that long), frame 1 none of class 3."""
    rng = np.random.default_rng(seed)
    anchors = make_anchors(fm[0], fm[1])
    dense = np.nonzero(anchors[:, 0] <= 2.0)[0]                 # the right part of the map stays free of ground truth
    frames, classes, importance = [], [], []
    for f, n in enumerate(counts):
        gt = _lattice_frame(rng, anchors, n, dense)
        cls = rng.choice([1, 3], n).astype(np.int32) if f != 1 else rng.choice([1, 2], n).astype(np.int32)
        if f == 0:
            cls[[i for i in (3, 100, 255, 256, 257, 280, n - 1) if 0 <= i < n]] = 2
        elif f > 1:
            cls[rng.random(n) < 0.3] = 2
        frames.append(gt); classes.append(cls)
        importance.append((rng.integers(4, 17, n) / 8).astype(np.float32))
    for gt in frames:
        assert_lattice_exact(anchors, gt, thresholds)
    stats = []
    big = int(np.argmax(counts))
    for m, u in thresholds:
        s = lattice_stats(anchors, frames[big], m, u)
        stats.append(s)
        if counts[big] >= 256:
            assert min(s["pos_thr"], s["forced_only"], s["background"], s["dont_care"]) >= 20, s
            assert s["forced_below_unmatched"] >= 1 and s["argmax_ties"] >= 5 and s["gt_no_overlap"] >= 3 and s["gt_duplicates"] >= 3, s
    return dict(anchors=anchors, gt=frames, classes=classes, importance=importance, stats=stats, thresholds=thresholds)


# ---------------------------------------------------------------------------------------------------------------------- loss
def dir_bin_margin(reg, anchors, labels, direction_offset, bins):
    """Smallest distance of off / (2 pi / bins) from an integer over the positive anchors (float64): off is the ground truth's
    rotation minus the offset, reduced to [0, 2 pi)."""
    rot = np.asarray(reg, np.float64)[..., 6] + np.asarray(anchors, np.float64)[None, :, 6] - direction_offset
    off = rot - np.floor(rot / (2 * np.pi)) * (2 * np.pi)
    q = off / (2 * np.pi / bins)
    d = np.abs(q - np.round(q))[np.asarray(labels) > 0]
    return d.min() if d.size else 1.0


def loss_case(seed, batch, n_anchor, num_class, bins, direction_offset=0.0, empty_frame=1, all_dont_care=False, logit_scale=6.0):
    """fp32 inputs of the loss: logits of scale ``logit_scale``, about 5 % positives (classes 1..num_class) and 5 % don't-care,
    frame ``empty_frame`` without a positive, importance in [0.5, 2].  Direction targets keep off / (2 pi / bins) at least 1e-4 from
    an integer (drawn again where they do not)."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    u = rng.random((batch, n_anchor))
    labels = np.where(u < 0.05, rng.integers(1, num_class + 1, (batch, n_anchor)), np.where(u < 0.10, -1, 0)).astype(np.int32)
    if n_anchor >= 8:
        labels[:, 0], labels[:, n_anchor - 1], labels[:, 1] = 1, num_class, -1          # the first and the last anchor count
    if empty_frame is not None and empty_frame < batch:
        labels[empty_frame][labels[empty_frame] > 0] = 0
    if all_dont_care:
        labels[:] = -1
    anchors = np.concatenate([f(n_anchor, 3) * 10, np.abs(f(n_anchor, 3)) + 1, rng.choice([0.0, np.pi / 2], (n_anchor, 1)).astype(np.float32)], 1)
    reg = f(batch, n_anchor, 7) * 0.5
    reg[..., 6] = rng.uniform(-3.5, 3.5, (batch, n_anchor)).astype(np.float32)
    if bins > 0:
        for _ in range(20):
            rot = reg[..., 6].astype(np.float64) + anchors[None, :, 6].astype(np.float64) - direction_offset
            q = (rot - np.floor(rot / (2 * np.pi)) * (2 * np.pi)) / (2 * np.pi / bins)
            bad = np.abs(q - np.round(q)) < 1e-4
            if not bad.any():
                break
            reg[..., 6][bad] = rng.uniform(-3.5, 3.5, int(bad.sum())).astype(np.float32)
    case = dict(cls=f(batch, n_anchor, num_class) * logit_scale, box=f(batch, n_anchor, 7) * 0.7, labels=labels, reg=reg,
                anchors=anchors.astype(np.float32), importance=rng.uniform(0.5, 2.0, (batch, n_anchor)).astype(np.float32))
    case["dir"] = f(batch, n_anchor, bins) * 2 if bins > 0 else None
    return case


def loss_ref(cls, box, dirp, labels, reg, anchors, importance, num_class=1, num_direction_bins=2, dtype=torch.float64, **cfg):
    """standin_loss on ``dtype`` tensors under autograd.  -> (out6, d_cls, d_box, d_dir) as numpy arrays of that precision with
    out6 = (loss, cls_loss_reduced, loc_loss_reduced, dir_loss_reduced, cls_pos_loss, cls_neg_loss); the gradients are those of
    `loss`.  num_direction_bins = 0: no direction head (dir_loss_reduced 0, d_dir None).  ``cfg``: entries of LOSS_DEFAULTS."""
    assert set(cfg) <= set(LOSS_KEYS), sorted(set(cfg) - set(LOSS_KEYS))
    p = dict(LOSS_DEFAULTS, **cfg)
    bins = int(num_direction_bins)
    if bins > 0:
        assert dir_bin_margin(reg, anchors, labels, p["direction_offset"], bins) >= 1e-4, "a direction target sits on a bin edge"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    b, n = np.asarray(labels).shape
    net = types.SimpleNamespace(
        _num_class=int(num_class), _pos_cls_weight=p["pos_cls_weight"], _neg_cls_weight=p["neg_cls_weight"],
        _cls_loss_weight=p["classification_weight"], _loc_loss_weight=p["localization_weight"],
        _direction_loss_weight=p["direction_loss_weight"], _sin_error_factor=p["sin_error_factor"],
        _cls_loss_ftor=_named("SigmoidFocalClassificationLoss", _alpha=p["alpha"], _gamma=p["gamma"]),
        _loc_loss_ftor=_named("WeightedSmoothL1LocalizationLoss", _sigma=p["sigma"], _codewise=True,
                              _code_weights=torch.tensor(p["code_weights"], dtype=dtype)),
        _use_direction_classifier=bins > 0, _num_direction_bins=bins, _dir_offset=p["direction_offset"])
    leaves = [t(cls).reshape(b, n, num_class).requires_grad_(), t(box).reshape(b, n, 7).requires_grad_()]
    preds = {"cls_preds": leaves[0], "box_preds": leaves[1]}
    if bins > 0:
        leaves.append(t(dirp).reshape(b, n, bins).requires_grad_())
        preds["dir_cls_preds"] = leaves[2]
    example = {"labels": torch.from_numpy(np.ascontiguousarray(labels)).int(), "reg_targets": t(reg), "importance": t(importance),
               "anchors": t(anchors).unsqueeze(0).expand(b, -1, -1)}
    res = standin_loss(net, example, preds)
    grads = torch.autograd.grad(res["loss"], leaves)
    zero = torch.zeros((), dtype=dtype)
    out6 = torch.stack([res["loss"], res["cls_loss_reduced"], res["loc_loss_reduced"], res.get("dir_loss_reduced", zero),
                        res["cls_pos_loss"], res["cls_neg_loss"]]).detach().numpy()
    g = [x.numpy() for x in grads]
    return out6, g[0], g[1], (g[2] if bins > 0 else None)


# --------------------------------------------------------------------------------------------------------------------- AdamW
def adamw_ref(p, m, v, g, step, lr, beta1, beta2, eps, weight_decay, max_grad_norm):
    """One clipped AdamW step in float64; ``step`` counts from 1.  -> (p, m, v, norm).
    norm = |g|; g *= min(1, max_norm / (norm + 1e-6)) unless max_norm <= 0; p *= 1 - lr wd; m += (g - m)(1 - b1);
    v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)."""
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, g))
    norm = float(np.sqrt(np.sum(g * g)))
    clip = min(1.0, max_grad_norm / (norm + 1e-6)) if max_grad_norm > 0 else 1.0
    g = g * clip
    p = p * (1.0 - lr * weight_decay)
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + g * g * (1.0 - beta2)
    p = p - lr / (1.0 - beta1 ** step) * (m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** step) + eps))
    return p, m, v, norm
