"""Host side of the KITTI AP evaluation tests: the fixture's layout, a numpy restatement of the four stages, hand-built cases.

tests/golden/kitti_eval.npz is recorded from the executed reference (tests/golden/make_golden_kitti_eval.py).  The restatement below
is this project's own text: the matching is vectorised the way the kernels are -- pass 1 as an arg-max over the detections of one gt,
pass 2 with one array element per score threshold -- and test_kitti_eval_host.py holds it to every recorded array, so the GPU tests
can use it where no fixture exists (the hand-built cases).  Overlaps of metrics 1 and 2 need the polygon clipper and are not restated:
hand-built cases use metric 0 or overlap blocks drawn at random (the matching takes any block).
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_eval.npz")
N_PTS = 41
MAX_GT = MAX_DT = 512                  # include/second_hip.h SEC_KITTI_EVAL_MAX_GT / _MAX_DT
CHUNK = 32                             # SEC_KITTI_EVAL_CHUNK
CLASS_NAMES = ['car', 'pedestrian', 'cyclist', 'van', 'person_sitting', 'car', 'tractor', 'trailer']
MIN_HEIGHT, MAX_OCCLUSION, MAX_TRUNCATION = [40, 25, 25], [0, 1, 2], [0.15, 0.3, 0.5]
CASES = {
    "A": dict(classes=["Car", "Pedestrian", "Cyclist"], class_ids=[0, 1, 2], z_axis=1, z_center=1.0, images=8, compute_aos=True),
    "B": dict(classes=["car"], class_ids=[5], z_axis=2, z_center=0.5, images=5, compute_aos=False),
}
DIFFICULTYS = [0, 1, 2]
GT_KEYS = ["name", "bbox", "alpha", "occluded", "truncated", "location", "dimensions", "rotation_y"]
DT_KEYS = ["name", "bbox", "alpha", "score", "location", "dimensions", "rotation_y"]
KINDS = ("official", "coco")


def official_min_overlaps(class_ids):
    """[2, 3 metrics, classes]: the two rows of KITTI's official thresholds (moderate / easy tables of get_official_eval_result)."""
    strict = {0: 0.7, 1: 0.5, 2: 0.5, 3: 0.7, 4: 0.5, 5: 0.7, 6: 0.7, 7: 0.7}
    loose_bbox = {0: 0.7, 1: 0.5, 2: 0.5, 3: 0.7, 4: 0.5, 5: 0.5, 6: 0.5, 7: 0.5}
    loose_3d = {0: 0.5, 1: 0.25, 2: 0.25, 3: 0.5, 4: 0.25, 5: 0.5, 6: 0.5, 7: 0.5}
    out = np.zeros((2, 3, len(class_ids)))
    for j, c in enumerate(class_ids):
        out[0, :, j] = strict[c]
        out[1, :, j] = [loose_bbox[c], loose_3d[c], loose_3d[c]]
    return out


def coco_min_overlaps(class_ids):
    """[10, 3, classes]: linspace(0.5, 0.95, 10) for the vehicle classes, linspace(0.25, 0.7, 10) for people and cyclists."""
    out = np.zeros((10, 3, len(class_ids)))
    for j, c in enumerate(class_ids):
        out[:, :, j] = (np.linspace(0.25, 0.7, 10) if c in (1, 2, 4) else np.linspace(0.5, 0.95, 10))[:, None]
    return out


def min_overlaps_of(kind, class_ids):
    return official_min_overlaps(class_ids) if kind == "official" else coco_min_overlaps(class_ids)


# ------------------------------------------------------------------------------------------------ fixture layout
def store_annos(out, prefix, annos, keys):
    out[prefix + "_num"] = np.array([len(a["name"]) for a in annos], np.int32)
    for k in keys:
        parts = [np.asarray(a[k]) for a in annos]
        out[f"{prefix}_{k}"] = np.concatenate(parts, 0) if k != "name" else np.array([n for a in annos for n in a["name"]], dtype="U16")


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def load_annos(g, prefix, keys):
    num = g[prefix + "_num"]
    off = np.concatenate([[0], np.cumsum(num)])
    return [{k: g[f"{prefix}_{k}"][off[i]:off[i + 1]] for k in keys} for i in range(len(num))]


def load_case(g, name):
    """-> dict(gt_annos, dt_annos, overlaps {metric: list of [dt_i, gt_i] float64 blocks}, flat {metric: float64 [n_ov]})."""
    gt, dt = load_annos(g, f"{name}_gt", GT_KEYS), load_annos(g, f"{name}_dt", DT_KEYS)
    sizes = [len(d["name"]) * len(t["name"]) for d, t in zip(dt, gt)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ov = {}
    for m in range(3):
        flat = g[f"{name}_overlaps_m{m}"]
        ov[m] = [flat[off[i]:off[i + 1]].reshape(len(dt[i]["name"]), len(gt[i]["name"])) for i in range(len(gt))]
    return dict(gt_annos=gt, dt_annos=dt, overlaps=ov, flat={m: np.ascontiguousarray(g[f"{name}_overlaps_m{m}"]) for m in range(3)})


def recorded(g, name, kind, metric):
    """The recorded arrays of one eval_class_v3 call, configurations ordered (class, difficulty, min_overlap)."""
    p = f"{name}_{kind}_m{metric}_"
    n_scores = g[p + "n_scores"]
    off = np.concatenate([[0], np.cumsum(n_scores)])
    return dict(compute_aos=bool(g[p + "compute_aos"]), n_scores=n_scores,
                scores=[g[p + "scores"][off[c]:off[c + 1]] for c in range(len(n_scores))],
                thresholds=g[p + "thresholds"], n_thresholds=g[p + "n_thresholds"], pr=g[p + "pr"],
                precision=g[p + "precision"], orientation=g[p + "orientation"])


def recorded_results(g, name):
    return {k: dict(result=str(g[f"{name}_{k}_result"]), detail=json.loads(str(g[f"{name}_{k}_detail"]))) for k in KINDS}


# ------------------------------------------------------------------------------------------------ the four stages in numpy
def image_overlap_np(boxes, query, criterion=-1):
    """[N, K] float64 overlap of (x1, y1, x2, y2) rows: intersection over union (-1) or over the area of ``boxes`` (0)."""
    b, q = boxes[:, None, :], query[None, :, :]
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0])
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1])
    barea = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    qarea = (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
    ua = barea + qarea - iw * ih if criterion == -1 else barea + 0 * qarea
    with np.errstate(divide="ignore", invalid="ignore"):
        v = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), v, 0.0)


def flags_np(gt, dt, class_id, difficulty):
    """(ignored_gt, ignored_dt, num_valid_gt) of one image for one class and difficulty; names are compared, not class indices."""
    cls = CLASS_NAMES[class_id]
    gname = np.char.lower(np.asarray(gt["name"], dtype="U16"))
    dname = np.char.lower(np.asarray(dt["name"], dtype="U16"))
    same = gname == cls
    neutral = ((cls == "pedestrian") & (gname == "person_sitting")) | ((cls == "car") & (gname == "van"))
    h = gt["bbox"][:, 3] - gt["bbox"][:, 1] if len(gname) else np.zeros(0)
    hard = (gt["occluded"] > MAX_OCCLUSION[difficulty]) | (gt["truncated"] > MAX_TRUNCATION[difficulty]) | (h <= MIN_HEIGHT[difficulty])
    ign_gt = np.where(same & ~hard, 0, np.where(same | neutral, 1, -1)).astype(np.int8)
    dh = np.abs(dt["bbox"][:, 3] - dt["bbox"][:, 1]) if len(dname) else np.zeros(0)
    ign_dt = np.where(dh < MIN_HEIGHT[difficulty], 1, np.where(dname == cls, 0, -1)).astype(np.int8)
    return ign_gt, ign_dt, int((ign_gt == 0).sum())


def tp_scores_np(overlap, scores, ign_gt, ign_dt, min_overlap):
    """Pass 1 on one image: for each gt in order the unassigned, not-excluded detection of highest score among those overlapping more
    than ``min_overlap`` (np.argmax: the first of equal scores); a pair with an ignored side is consumed without a score."""
    free = ign_dt != -1
    out = []
    for i in np.flatnonzero(ign_gt != -1):
        elig = free & (overlap[:, i] > min_overlap) & (scores > -10000000)
        if not elig.any():
            continue
        j = int(np.argmax(np.where(elig, scores, -np.inf)))
        free = free.copy()
        free[j] = False
        if ign_gt[i] == 0 and ign_dt[j] == 0:
            out.append(scores[j])
    return np.array(out, np.float64)


def thresholds_np(sorted_scores, num_gt):
    """The recall sampling: walk the descending scores, keep one whenever the running recall target (steps of 1 / 40, accumulated in
    float64) is nearer to this score's recall than to the next one's."""
    n = len(sorted_scores)
    target, out = 0.0, []
    for i in range(n):
        left = (i + 1) / num_gt
        right = (i + 2) / num_gt if i < n - 1 else left
        if i < n - 1 and (right - target) < (target - left):
            continue
        out.append(sorted_scores[i])
        target += 1 / 40.0
    return np.array(out, np.float64)


def pr_np(overlap, gt, dt, ign_gt, ign_dt, dc_bbox, metric, min_overlap, thresholds, compute_aos, counters=None):
    """Pass 2 on one image, one array element per threshold: -> (tp, fp, fn int64 [T], similarity float64 [T])."""
    T, nd = len(thresholds), len(ign_dt)
    scores = dt["score"]
    live = (scores[None, :] >= thresholds[:, None]) & (ign_dt != -1)[None, :] if nd else np.zeros((T, 0), bool)   # [T, nd], not yet assigned
    counted = live & (ign_dt == 0)[None, :]                                # what can become a false positive
    tp, fn, sim = np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T)
    rows = np.arange(T)
    for i in np.flatnonzero(ign_gt != -1):
        if nd == 0:
            fn += int(ign_gt[i] == 0)
            continue
        det = np.full(T, -1)
        best = np.zeros(T)
        holds_ignored = np.zeros(T, bool)
        for j in np.flatnonzero((ign_dt != -1) & (overlap[:, i] > min_overlap)) if nd else []:
            ov, can = overlap[j, i], live[:, j]
            if ign_dt[j] == 0:
                take = can & ((ov > best) | holds_ignored)
                if counters is not None and (can & holds_ignored).any():
                    counters["replaced_ignored_det"] = counters.get("replaced_ignored_det", 0) + 1
                best = np.where(take, ov, best)
                holds_ignored &= ~take
            else:
                take = can & (det < 0)
                holds_ignored |= take
            det = np.where(take, j, det)
        found = det >= 0
        fn += ~found & (ign_gt[i] == 0)
        hit = found & (ign_gt[i] == 0) & (ign_dt[np.maximum(det, 0)] == 0)
        tp += hit
        if compute_aos and hit.any():
            sim += np.where(hit, (1.0 + np.cos(gt["alpha"][i] - dt["alpha"][np.maximum(det, 0)])) / 2.0, 0.0)
        live[rows[found], det[found]] = False
    left = live & counted
    if metric == 0 and len(dc_bbox) and nd:
        inside = (image_overlap_np(dt["bbox"], dc_bbox, 0) > min_overlap).any(1)
        if counters is not None:
            counters["nstuff"] = counters.get("nstuff", 0) + int((left & inside[None, :]).sum())
        left = left & ~inside[None, :]
    return tp, left.sum(1), fn, sim


def eval_np(gt_annos, dt_annos, overlaps, class_ids, difficultys, metric, min_overlaps, compute_aos=False, counters=None):
    """All stages for one call -> dict: ignored_gt / ignored_dt [ncd, n], num_valid_gt [ncd], scores (list per configuration, descending),
    thresholds [configs, 41], n_thresholds, pr [configs, 41, 4] float64, precision / orientation [class, difficulty, k, 41]."""
    num_k, ncls, ndiff = min_overlaps.shape[0], len(class_ids), len(difficultys)
    configs = ncls * ndiff * num_k
    res = dict(ignored_gt=[], ignored_dt=[], num_valid_gt=[], scores=[], thresholds=np.zeros((configs, N_PTS)),
               n_thresholds=np.zeros(configs, np.int32), pr=np.zeros((configs, N_PTS, 4)))
    dcs = [g["bbox"][np.asarray(g["name"], dtype="U16") == "DontCare"].reshape(-1, 4) for g in gt_annos]
    for m, c in enumerate(class_ids):
        for l, d in enumerate(difficultys):
            fl = [flags_np(g, t, c, d) for g, t in zip(gt_annos, dt_annos)]
            res["ignored_gt"].append(np.concatenate([f[0] for f in fl]) if fl else np.zeros(0, np.int8))
            res["ignored_dt"].append(np.concatenate([f[1] for f in fl]) if fl else np.zeros(0, np.int8))
            nvg = sum(f[2] for f in fl)
            res["num_valid_gt"].append(nvg)
            for k in range(num_k):
                cfg, mo = (m * ndiff + l) * num_k + k, min_overlaps[k, metric, m]
                sc = [tp_scores_np(overlaps[i], dt_annos[i]["score"], fl[i][0], fl[i][1], mo) for i in range(len(gt_annos))]
                sc = np.sort(np.concatenate(sc) if sc else np.zeros(0))[::-1]
                res["scores"].append(sc)
                th = thresholds_np(sc, nvg)
                res["n_thresholds"][cfg] = len(th)
                res["thresholds"][cfg, :len(th)] = th
                for i in range(len(gt_annos)):
                    tp, fp, fn, sim = pr_np(overlaps[i], gt_annos[i], dt_annos[i], fl[i][0], fl[i][1], dcs[i], metric, mo, th, compute_aos,
                                            counters)
                    res["pr"][cfg, :len(th)] += np.stack([tp, fp, fn, sim], 1)
    res["ignored_gt"], res["ignored_dt"] = np.stack(res["ignored_gt"]), np.stack(res["ignored_dt"])
    res["num_valid_gt"] = np.array(res["num_valid_gt"], np.int32)
    res["precision"], res["orientation"] = finish_np(res["pr"], res["n_thresholds"], (ncls, ndiff, num_k), compute_aos)
    return res


def finish_np(pr, n_thresholds, shape, compute_aos):
    """precision = tp / (tp + fp) and aos = similarity / (tp + fp) over the first n_thresholds points, then the maximum over
    everything to the right (the zeros behind n included; a NaN from 0 / 0 spreads left, as np.max does)."""
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for col in ((0, 3) if compute_aos else (0,)):
            v = np.zeros(pr.shape[:2])
            for c, n in enumerate(n_thresholds):
                v[c, :n] = pr[c, :n, col] / (pr[c, :n, 0] + pr[c, :n, 1])
                v[c, :n] = np.maximum.accumulate(v[c, ::-1])[::-1][:n]
            out.append(v.reshape(*shape, N_PTS))
    if not compute_aos:
        out.append(np.zeros(shape + (N_PTS,)))
    return out[0], out[1]


def similarity_bound(pr):
    """|error| allowed on a similarity sum: n * 2^-52 * S with n the number of terms (tp) and S the sum -- (n - 1) roundings of the
    float64 summation plus one ulp for each cosine."""
    return pr[..., 0] * 2.0 ** -52 * pr[..., 3]


# ------------------------------------------------------------------------------------------------ hand-built cases
def random_annos(rng, images, n_gt, n_dt, classes=("Car",), dontcare=0, tie_scores=False, score_range=(0.05, 1.0)):
    """Camera-format annotation dicts whose bbox overlaps (metric 0) exercise the matching: ``n_gt`` / ``n_dt`` are per-image counts
    (ints or per-image lists).  Detections are jittered gt boxes and free boxes; scores are multiples of 1 / 64 when ``tie_scores``."""
    n_gt = [n_gt] * images if np.isscalar(n_gt) else list(n_gt)
    n_dt = [n_dt] * images if np.isscalar(n_dt) else list(n_dt)
    names = list(classes) + ["Van", "Person_sitting"]
    gts, dts = [], []
    for g, d in zip(n_gt, n_dt):
        xy = rng.uniform(0, 900, (g + dontcare, 2))
        wh = np.stack([rng.uniform(30, 90, g + dontcare), rng.choice([20.0, 30.0, 45.0, 60.0, 80.0], g + dontcare)], 1)
        gname = [names[int(i)] for i in rng.choice(len(names), g, p=[0.8 / len(classes)] * len(classes) + [0.1, 0.1])] + ["DontCare"] * dontcare
        gt = dict(name=np.array(gname, dtype="U16"), bbox=np.concatenate([xy, xy + wh], 1), alpha=rng.uniform(-3, 3, g + dontcare),
                  occluded=rng.choice([0, 0, 0, 1, 2, 3], g + dontcare).astype(np.int64), truncated=rng.choice([0.0, 0.0, 0.0, 0.2, 0.4, 0.6], g + dontcare),
                  location=rng.uniform(-10, 10, (g + dontcare, 3)), dimensions=rng.uniform(1, 3, (g + dontcare, 3)),
                  rotation_y=rng.uniform(-3, 3, g + dontcare))
        src = rng.integers(0, max(g + dontcare, 1), d) if g + dontcare else np.zeros(d, np.int64)
        free = rng.random(d) < 0.25 if g + dontcare else np.ones(d, bool)
        base = gt["bbox"][src] if g + dontcare else np.zeros((d, 4))
        box = np.where(free[:, None], np.concatenate([(p := rng.uniform(0, 900, (d, 2))), p + rng.uniform(15, 80, (d, 2))], 1),
                       base + rng.normal(0, 1.5, (d, 4)))
        score = rng.integers(3, 65, d) / 64.0 if tie_scores else rng.uniform(*score_range, d)
        any_class = [classes[int(i)] for i in rng.integers(0, len(classes), d)]          # a copy keeps its object's name where that is a class
        dname = [gname[k] if (g + dontcare and not f and gname[k] in classes) else a for k, f, a in zip(src, free, any_class)]
        dt = dict(name=np.array(dname, dtype="U16"), bbox=box,
                  alpha=rng.uniform(-3, 3, d), score=score.astype(np.float64), location=rng.uniform(-10, 10, (d, 3)),
                  dimensions=rng.uniform(1, 3, (d, 3)), rotation_y=rng.uniform(-3, 3, d))
        gts.append(gt); dts.append(dt)
    return gts, dts


def bbox_overlaps(gt_annos, dt_annos):
    return [image_overlap_np(d["bbox"].reshape(-1, 4), g["bbox"].reshape(-1, 4)) for g, d in zip(gt_annos, dt_annos)]
