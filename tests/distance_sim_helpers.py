"""References for the DistanceSimilarity target assignment (csrc/train.hip: Sim<SEC_SIM_DISTANCE>, k_region_similarity).

  distance_similarity_ref   the similarity matrix, restated in vectorised numpy in BOTH arithmetic meanings of the formula
                              s = 0 unless |dx| <= dist_norm and |dy| <= dist_norm;  d = dx*dx + dy*dy;  x = min(d / dist_norm, dist_norm)
                              s = 1 - x      or, with rotation,      1 - (1 - rot_alpha) * x - rot_alpha * |sin(r_n - r_k)|
                            "compiled": what a jit compiler that types dist_norm / rot_alpha as float64 runs -- the differences, d and
                              |sin| are float32, the window tests and everything from the division on float64, ONE rounding into the
                              float32 matrix.  This is what the kernels implement.
                            "float32": what plain Python on numpy >= 2 float32 scalars runs (Python floats are weak): the chain is
                              float32 with float32(dist_norm) -- except where min() picks dist_norm, a Python float, after which the
                              arithmetic is float64 up to the next float32 operand.  tests/golden/distance_similarity.npz was
                              produced this way; test_distance_sim_host.py checks bit equality.
  meanings_bound            how far the two meanings can lie apart, per element (derivation in its docstring)
  assign_sim_ref / assign_ranges_ref   the matching of train_ref_helpers (_match, box_encode) on a similarity matrix
  decision_margin           how far a frame's decisions are from flipping
"""
import numpy as np

import train_ref_helpers as T

F32, F64 = np.float32, np.float64


def xyr(boxes):
    """[N, 7] boxes -> float32 (x, y, r), the columns DistanceSimilarity reads."""
    return np.ascontiguousarray(np.asarray(boxes, F32).reshape(-1, 7)[:, [0, 1, 6]])


def distance_similarity_ref(points, qpoints, dist_norm, with_rotation=False, rot_alpha=0.5, meaning="compiled"):
    """points [N, 3], qpoints [K, 3] float32 (x, y, r) -> [N, K] float32."""
    assert meaning in ("compiled", "float32")
    p, q = np.asarray(points, F32), np.asarray(qpoints, F32)
    assert p.dtype == F32 and q.dtype == F32
    dn, ra = float(dist_norm), float(rot_alpha)
    ra1 = 1 - ra
    dx = p[:, None, 0] - q[None, :, 0]
    dy = p[:, None, 1] - q[None, :, 1]
    d = dx * dx + dy * dy
    rot = np.abs(np.sin(p[:, None, 2] - q[None, :, 2])) if with_rotation else np.zeros_like(d)
    assert d.dtype == F32 and rot.dtype == F32
    if meaning == "compiled":
        inside = (np.abs(dx).astype(F64) <= dn) & (np.abs(dy).astype(F64) <= dn)
        x = np.minimum(d.astype(F64) / dn, dn)
        s = 1.0 - ra1 * x - ra * rot.astype(F64) if with_rotation else 1.0 - x
        assert s.dtype == F64
        return np.where(inside, s, 0.0).astype(F32)
    dn32 = F32(dn)
    inside = (np.abs(dx) <= dn32) & (np.abs(dy) <= dn32)
    xq = d / dn32                                           # float32 / weak Python float
    clamp = dn32 < xq                                       # min(a, b) keeps a unless b < a; b is then the PYTHON float dist_norm
    if with_rotation:
        free = (F32(1) - F32(ra1) * xq) - F32(ra) * rot     # all float32
        held = F32(1 - ra1 * dn) - F32(ra) * rot            # 1 - rot_alpha_1 * dist_norm is a Python float until it meets float32
    else:
        free = F32(1) - xq
        held = np.full_like(xq, F32(1 - dn))                # float64 difference, rounded on the store
    s = np.where(clamp, held, free)
    assert s.dtype == F32
    return np.where(inside, s, F32(0)).astype(F32)


def meanings_bound(points, qpoints, dist_norm, with_rotation=False, rot_alpha=0.5):
    """[N, K] float64: an upper bound of |compiled - float32| wherever both meanings put the pair on the same side of the window.

    u = 2^-24 (float32 unit roundoff).  float32(dist_norm) = dist_norm (1 + e0), |e0| <= u.
      x:   the float32 chain rounds the quotient by the rounded norm: x32 = x (1 + e1) / (1 + e0), so |x32 - x| <= 2u x (1 + u);
           where the min picks dist_norm both meanings hold the same float64 number and the difference is 0.
      no rotation:  float32: fl(1 - x32); compiled: fl(1 - x).  Each rounds once, by at most half an ulp of a neighbour of s:
                    |diff| <= 2u x (1 + u) + ulp32(s'),   s' = |s| + 2u x (the larger of the two magnitudes).
      rotation:     a1 = 1 - rot_alpha.  float32: t = fl(fl(a1) * x32) errs by <= a1 x (4u)(1 + 2u); fl(1 - t) adds half an ulp of
                    |1 - t| <= max(1, |1 - a1 x|) -> <= u * max(1, |1 - a1 x|) * 2 (ulp of the next binade up, to be safe);
                    v = fl(fl(rot_alpha) * rot) errs by <= rot_alpha * rot * 2u (1 + u); the final difference and the compiled store
                    round once each: ulp32(s').  The sine is the same float32 number in both.
    The clamped elements still carry the rotation and rounding terms."""
    p, q = np.asarray(points, F32).astype(F64), np.asarray(qpoints, F32).astype(F64)
    dn, ra = float(dist_norm), float(rot_alpha)
    u = 2.0 ** -24
    dx32 = np.asarray(points, F32)[:, None, :] - np.asarray(qpoints, F32)[None, :, :]
    d = (dx32[..., 0] * dx32[..., 0] + dx32[..., 1] * dx32[..., 1]).astype(F64)
    x = np.minimum(d / dn, dn)
    ex = np.where(d / dn * (1 - 4 * u) > dn, 0.0, 2 * u * x * (1 + u))          # 0 where both meanings clearly clamp
    if not with_rotation:
        s = np.abs(1 - x) + ex
        return ex + np.spacing(s.astype(F32)).astype(F64)
    rot = np.abs(np.sin(dx32[..., 2])).astype(F64)
    a1 = 1 - ra
    et = np.where(ex > 0, a1 * x * 4 * u * (1 + 2 * u), 0.0)                    # clamped: 1 - a1 * dist_norm is float64, rounded once (e1)
    e1 = 2 * u * np.maximum(1.0, np.abs(1 - a1 * x))
    ev = ra * rot * 2 * u * (1 + u)
    s = np.abs(1 - a1 * x - ra * rot) + et + e1 + ev
    return et + e1 + ev + np.spacing(s.astype(F32)).astype(F64)


def similarity_matrix(anchors, gt, sim, meaning="compiled"):
    """[N, 7] x [K, 7] -> [N, K] float64 under ``sim``: None / "nearest_iou" (train_ref_helpers' float64 near-box IoU) or
    dict(kind="distance", distance_norm=, with_rotation=, rotation_alpha=)."""
    if sim is None or sim == "nearest_iou":
        return T.iou_eps0(T.near_boxes(anchors), T.near_boxes(gt))
    assert sim["kind"] == "distance"
    return distance_similarity_ref(xyr(anchors), xyr(gt), sim["distance_norm"], sim.get("with_rotation", False),
                                   sim.get("rotation_alpha", 0.5), meaning).astype(F64)


def assign_sim_ref(anchors, gt, sim, matched, unmatched, gt_classes=None, gt_importance=None, mask=None, gmax=None,
                   importance_table=None, meaning="compiled"):
    """train_ref_helpers.assign_ref with the overlaps replaced by ``similarity_matrix(sim)``: same matching (_match: first-index
    argmax, the -1 fill of a zero column maximum, ties with a column maximum forced positive -- with NO guard against negative
    similarities, as in the reference), same box encoding.  -> labels, targets, importance, info (+ the matrix as info["sim"])."""
    anchors, gt = np.asarray(anchors, F32), np.asarray(gt, F32).reshape(-1, 7)
    n = len(anchors)
    keep = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    labels, targets, imp = np.full(n, -1, np.int32), np.zeros((n, 7)), np.where(keep, 1.0, 0.0).astype(F32)
    info = dict(max=np.full(n, -np.inf), arg=np.full(n, -1), pos=np.zeros(n, bool), force=np.zeros(n, bool), sim=None, gmax=None)
    if len(gt) == 0:
        labels[keep] = 0
        return labels, targets, imp, info
    classes = np.ones(len(gt), np.int32) if gt_classes is None else np.asarray(gt_classes, np.int32)
    table = importance_table if importance_table is not None else gt_importance
    ov = similarity_matrix(anchors[keep], gt, sim, meaning)
    if gmax is None:
        gmax = ov.max(0) if len(ov) else np.full(len(gt), np.nan)
    lab, arg, mx, pos, force = T._match(ov, gmax, np.broadcast_to(matched, (n,))[keep], np.broadcast_to(unmatched, (n,))[keep], classes)
    idx = np.nonzero(keep)[0]
    labels[idx] = lab
    if table is not None:
        imp[idx[pos]] = np.asarray(table, F32)[arg[pos]]
    fg = lab > 0
    targets[idx[fg]] = T.box_encode(gt[arg[fg]], anchors[idx[fg]])
    for k, v in (("max", mx), ("arg", arg), ("pos", pos), ("force", force)):
        info[k][idx] = v
    info["sim"], info["gmax"] = ov, np.where(gmax == 0, -1.0, gmax)
    return labels, targets, imp, info


def assign_ranges_ref(anchors, gt, gt_classes, begins, class_ids, matched, unmatched, sims, gt_importance=None, mask=None,
                      meaning="compiled", want_info=False):
    """train_ref_helpers.assign_per_class_ref with a similarity per range (``sims[c]`` as in similarity_matrix).  class_ids[c] = 0
    (assign_all): the similarity of range 0 for every such range, a ground truth's maximum taken over the anchors of all of them."""
    anchors, gt = np.asarray(anchors, F32), np.asarray(gt, F32).reshape(-1, 7)
    gt_classes = np.asarray(gt_classes, np.int32)
    n = len(anchors)
    labels, targets, imp = np.full(n, -1, np.int32), np.zeros((n, 7)), np.ones(n, F32)
    keep = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    infos = []
    gmax_all = None
    if len(gt) and any(k == 0 for k in class_ids):
        live = np.zeros(n, bool)
        for c, k in enumerate(class_ids):
            if k == 0:
                live[begins[c]:begins[c + 1]] = True
        ov = similarity_matrix(anchors[live & keep], gt, sims[0], meaning)
        gmax_all = ov.max(0) if len(ov) else np.full(len(gt), np.nan)
    for c, k in enumerate(class_ids):
        s = slice(begins[c], begins[c + 1])
        if begins[c] == begins[c + 1]:
            infos.append(None)
            continue
        m = None if mask is None else keep[s]
        if k == 0:
            l, t, i, info = assign_sim_ref(anchors[s], gt, sims[0], matched[c], unmatched[c], gt_classes, gt_importance, m,
                                           gmax=gmax_all, meaning=meaning)
        else:
            sel = gt_classes == k
            l, t, i, info = assign_sim_ref(anchors[s], gt[sel], sims[c], matched[c], unmatched[c], gt_classes[sel], gt_importance, m,
                                           meaning=meaning)
        labels[s], targets[s], imp[s] = l, t, i
        infos.append(info)
    return (labels, targets, imp, infos) if want_info else (labels, targets, imp)


def decision_margin(sim, gmax, matched, unmatched):
    """The smallest distance of any anchor's best similarity (row maximum of ``sim`` [N, K]) from either threshold, and of any
    similarity from its ground truth's maximum ``gmax`` [K] (after the -1 fill) where the two are not bit-equal.  inf for an empty
    matrix.  A perturbation of every similarity by less than half of it changes no decision of the matching."""
    sim = np.asarray(sim, F64)
    if sim.size == 0:
        return np.inf
    best = sim.max(1)
    m = min(np.abs(best - F64(matched)).min(), np.abs(best - F64(unmatched)).min())
    g = np.asarray(gmax, F64)[None, :]
    d = np.abs(sim - g)
    d = d[(sim != g) & np.isfinite(d)]
    return float(min(m, d.min())) if d.size else float(m)


def argmax_margin(sim):
    """The smallest gap between a row's maximum and the entries of that row that are not bit-equal to it."""
    sim = np.asarray(sim, F64)
    if sim.size == 0 or sim.shape[1] < 2:
        return np.inf
    d = sim.max(1, keepdims=True) - sim
    d = d[d > 0]
    return float(d.min()) if d.size else np.inf


# ------------------------------------------------------------------------------------------- tests/golden/distance_similarity.npz
FIXTURE_CLASSES = ["car", "pedestrian", "cyclist"]


def fixture_sims(g, tag):
    """The similarity of every anchor generator in mode ``tag`` ("per_class", "all", "all_dist"), as similarity_matrix takes it."""
    out = []
    for i in g[f"calculators_{tag}"].tolist():
        kind, dn, rot, alpha = g[f"sim_{i}"].tolist()
        out.append(None if kind == 0 else dict(kind="distance", distance_norm=dn, with_rotation=bool(rot), rotation_alpha=alpha))
    return out


def fixture_frames(g):
    n = int(g["frames"])
    return [(g[f"gt_{f}"], g[f"gt_classes_{f}"], g[f"gt_importance_{f}"]) for f in range(n)]


def fixture_expected(g, tag):
    """labels int32 [F, A], bbox_targets float32 [F, A, 7], importance float32 [F, A] of mode ``tag`` (stored sparsely)."""
    labels = g[f"labels_{tag}"].astype(np.int32)
    targets = np.zeros(labels.shape + (7,), F32)
    importance = np.ones(labels.shape, F32)
    rows = g[f"target_rows_{tag}"]
    targets[rows[:, 0], rows[:, 1]] = g[f"target_vals_{tag}"]
    importance[rows[:, 0], rows[:, 1]] = g[f"importance_pos_{tag}"]
    return labels, targets, importance


class NearestIouSimilarity:                         # stand-ins: the attribute and class names similarity_config reads
    pass


class RotateIouSimilarity:
    pass


class DistanceSimilarity:
    def __init__(self, distance_norm, with_rotation=False, rotation_alpha=0.5):
        self._distance_norm, self._with_rotation, self._rotation_alpha = distance_norm, with_rotation, rotation_alpha


class GroundBox3dCoder:
    code_size = 7

    def __init__(self, linear_dim=False, vec_encode=False):
        self.linear_dim, self.vec_encode = linear_dim, vec_encode


class _Generator:
    def __init__(self, class_name, match_threshold, unmatch_threshold):
        self.class_name, self.match_threshold, self.unmatch_threshold = class_name, match_threshold, unmatch_threshold


class StandinTargetAssigner:
    """Shaped like second.core.target_assigner.TargetAssigner as far as second_amd.targets reads it; the anchors come from a
    table instead of the generators."""

    def __init__(self, classes, generators, calculators, assign_per_class, anchors_by_class, positive_fraction=None, box_coder=None):
        self._classes, self._anchor_generators, self._sim_calcs = classes, generators, calculators
        self._assign_per_class, self._positive_fraction = assign_per_class, positive_fraction
        self._box_coder = box_coder or GroundBox3dCoder()
        self._anchors_by_class = anchors_by_class

    def generate_anchors_dict(self, feature_map_size):
        return {g.class_name: {"anchors": self._anchors_by_class[g.class_name]} for g in self._anchor_generators}


def standin_assigner(g, tag, **kw):
    """The fixture's TargetAssigner of mode ``tag`` as a stand-in object."""
    begin = g["class_anchor_begin"].tolist()
    gens = [_Generator(c, float(m), float(u)) for c, m, u in zip(FIXTURE_CLASSES, g["matched"].astype(F64), g["unmatched"].astype(F64))]
    calcs = [NearestIouSimilarity() if s is None else DistanceSimilarity(s["distance_norm"], s["with_rotation"], s["rotation_alpha"])
             for s in fixture_sims(g, tag)]
    table = {c: g["anchors"][begin[i]:begin[i + 1]] for i, c in enumerate(FIXTURE_CLASSES)}
    return StandinTargetAssigner(list(FIXTURE_CLASSES), gens, calcs, tag == "per_class", table, **kw)
