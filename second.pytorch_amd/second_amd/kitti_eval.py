"""``eval_class_v3`` of second/utils/eval.py (:479-611) on the device.

The reference's KITTI AP evaluation is numba-jitted host code around one GPU kernel (the rotated IoU); without numba its loops run as
plain Python.  Here the four stages -- per-image overlap blocks, clean_data's ignore flags, the true-positive scores
(compute_statistics_jit without fp), get_thresholds and the PR statistics (fused_compute_statistics) -- run as ``sec_kitti_eval_*``
kernels for all classes, difficulties and min_overlaps of a call at once; the host packs the annotation dicts once per call and
finishes exactly as the reference does (precision = tp / (tp + fp) in float64, running maximum from the right).

``compat.accelerate_eval(statistics=True)`` (or SEC_EVAL_DEVICE=1) installs :func:`eval_class_v3` as ``second.utils.eval.eval_class_v3``;
``do_eval_v2`` / ``do_eval_v3`` resolve the name at call time, so ``get_official_eval_result`` and ``get_coco_eval_result`` (and
through them ``KittiDataset.evaluation`` / ``NuScenesDataset.evaluation_kitti``) use it unchanged.
"""
import numpy as np

# clean_data's table (eval.py:34-37) -- 'car' is in it twice, so classes are compared by NAME -- and the ids of include/second_hip.h
CLASS_NAMES = ['car', 'pedestrian', 'cyclist', 'van', 'person_sitting', 'car', 'tractor', 'trailer']
NAME_IDS = {'car': 0, 'pedestrian': 1, 'cyclist': 2, 'van': 3, 'person_sitting': 4, 'tractor': 5, 'trailer': 6}
NAME_OTHER = 7
N_SAMPLE_PTS = 41

# calls served by the device, and calls handed to the reference's eval_class_v3 because an image exceeds a cap
stats = {"device": 0, "fallback": 0}


def _name_ids(names):
    return np.array([NAME_IDS.get(str(n).lower(), NAME_OTHER) for n in names], np.int32)


def _cat(annos, key, cols=None, dtype=np.float64):
    parts = [np.asarray(a[key], dtype=dtype).reshape((-1,) if cols is None else (-1, cols)) for a in annos]
    shape = (0,) if cols is None else (0, cols)
    return np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros(shape, dtype))


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    assert off[-1] < 2 ** 31, "int32 offsets"
    return off.astype(np.int32)


def pack(gt_annos, dt_annos):
    """The annotation dicts (kitti_common.get_label_annos format) as flat float64 / int32 numpy arrays with per-image offsets.
    ``dt_annos`` a ``kitti_annos.DeviceAnnoList`` that is still as it was built (its ``handoff()``): the detection side is not packed
    again -- see :func:`_pack_handoff`."""
    assert len(gt_annos) == len(dt_annos)
    handoff = getattr(dt_annos, "handoff", None)
    held = handoff() if callable(handoff) else None
    if held is not None:
        return _pack_handoff(gt_annos, dt_annos, held)
    gt_num = np.array([len(a["name"]) for a in gt_annos], np.int64)
    dt_num = np.array([len(a["name"]) for a in dt_annos], np.int64)
    gt_names = [n for a in gt_annos for n in a["name"]]
    p = {
        "images": len(gt_annos),
        "gt_off": _offsets(gt_num), "dt_off": _offsets(dt_num), "ov_off": _offsets(gt_num * dt_num),
        "max_gt": int(gt_num.max(initial=0)), "max_dt": int(dt_num.max(initial=0)),
        "gt_name": _name_ids(gt_names), "dt_name": _name_ids([n for a in dt_annos for n in a["name"]]),
        "gt_bbox": _cat(gt_annos, "bbox", 4), "dt_bbox": _cat(dt_annos, "bbox", 4),
        "gt_alpha": _cat(gt_annos, "alpha"), "dt_alpha": _cat(dt_annos, "alpha"), "dt_score": _cat(dt_annos, "score"),
        "gt_occluded": _cat(gt_annos, "occluded"), "gt_truncated": _cat(gt_annos, "truncated"),
    }
    for side, annos in (("gt", gt_annos), ("dt", dt_annos)):
        p[side + "_box3d"] = np.ascontiguousarray(np.concatenate(
            [_cat(annos, "location", 3), _cat(annos, "dimensions", 3), _cat(annos, "rotation_y")[:, None]], 1))
    dontcare = np.array([n == "DontCare" for n in gt_names], bool)               # case-sensitive, as clean_data
    p["dc_bbox"] = np.ascontiguousarray(p["gt_bbox"][dontcare])
    p["dc_off"] = _offsets(np.array([int(dontcare[a:b].sum()) for a, b in zip(p["gt_off"][:-1], p["gt_off"][1:])], np.int64))
    return p


_NO_DETECTIONS = {"name": np.zeros(0, "U1"), "bbox": np.zeros((0, 4)), "alpha": np.zeros(0), "score": np.zeros(0), "location": np.zeros((0, 3)),
                  "dimensions": np.zeros((0, 3)), "rotation_y": np.zeros(0)}


def _pack_handoff(gt_annos, dt_annos, held):
    """:func:`pack` for detections that are on the device already (``held``: dt_bbox, dt_alpha, dt_score, dt_box3d, dt_name, dt_off as
    device tensors, dt_num / max_dt on the host).  The gt side is packed by the plain route against images without detections; the
    dt_* arrays are left out of the result and the tensors travel under ``"_device"``, where :func:`run_stages` also leaves what it
    uploads.  The result is cached on the list, keyed by the identity and length of ``gt_annos``: the six eval_class_v3 calls of a val
    pass (get_official_eval_result, get_coco_eval_result) pack and upload the gt once."""
    cache = dt_annos.pack_cache
    if cache is not None and cache[0] is gt_annos and cache[1] == len(gt_annos):
        return cache[2]
    p = pack(gt_annos, [_NO_DETECTIONS] * len(gt_annos))
    for k in ("dt_name", "dt_bbox", "dt_alpha", "dt_score", "dt_box3d"):
        del p[k]
    dt_num = np.asarray(held["dt_num"], np.int64)
    p["dt_off"], p["max_dt"] = _offsets(dt_num), int(held["max_dt"])
    p["ov_off"] = _offsets(np.diff(p["gt_off"].astype(np.int64)) * dt_num)
    p["_device"] = {k: held[k] for k in ("dt_name", "dt_bbox", "dt_alpha", "dt_score", "dt_box3d", "dt_off")}
    dt_annos.pack_cache = (gt_annos, len(gt_annos), p)
    return p


def _reference_eval_class_v3():
    """The reference's own eval_class_v3: the original kept by compat.accelerate_eval, else the module's."""
    import importlib
    ev = importlib.import_module("second.utils.eval")
    return getattr(ev, "_second_amd_original_eval_class_v3", ev.eval_class_v3)


def class_difficulty_pairs(current_classes, difficultys):
    """(name ids, difficulties) of the flag planes, class-major: plane = class position * len(difficultys) + difficulty position."""
    names = [NAME_IDS[CLASS_NAMES[int(c)].lower()] for c in current_classes for _ in difficultys]
    diffs = [int(d) for _ in current_classes for d in difficultys]
    return names, diffs


def run_stages(p, current_classes, difficultys, metric, min_overlaps, compute_aos, z_axis, z_center, device=None, overlaps=None):
    """The four device stages on a :func:`pack` result.  ``overlaps``: use these blocks (a float64 tensor [n_ov]) instead of computing
    them.  -> dict of device tensors (overlaps, ignored_gt, ignored_dt, num_valid_gt, tp_scores, tp_count, sorted_scores, n_scores,
    thresholds, n_thresholds, counts, similarity) with configurations ordered (class, difficulty, min_overlap)."""
    import torch
    from . import ops
    dev = torch.device(device if device is not None else "cuda")
    held = p.get("_device")                                             # a hand-off pack: tensors that are on the device already
    t = {k: torch.from_numpy(v).to(dev) for k, v in p.items() if isinstance(v, np.ndarray) and (held is None or k not in held)}
    if held is not None:
        held.update(t)                                                  # the gt side is uploaded once per cached pack
        t = {k: v.to(dev) for k, v in held.items()}
    metric = int(metric)
    min_overlaps = np.asarray(min_overlaps, np.float64)
    num_k = min_overlaps.shape[0]
    n_ov = int(p["ov_off"][-1])
    out = {}
    if overlaps is None:
        boxes = ("dt_bbox", "gt_bbox") if metric == 0 else ("dt_box3d", "gt_box3d")
        overlaps = ops.kitti_eval_overlaps(metric, t["dt_off"], t["gt_off"], t["ov_off"], t[boxes[0]], t[boxes[1]], n_ov, p["max_dt"], p["max_gt"],
                                           z_axis, z_center)
    out["overlaps"] = overlaps
    names, diffs = class_difficulty_pairs(current_classes, difficultys)
    ign_gt, ign_dt, nvg = ops.kitti_eval_flags(names, diffs, t["gt_name"], t["gt_bbox"], t["gt_occluded"], t["gt_truncated"], t["dt_name"],
                                               t["dt_bbox"])
    out["ignored_gt"], out["ignored_dt"], out["num_valid_gt"] = ign_gt, ign_dt, nvg
    # cfg = (class, difficulty, k): min_overlaps[k, metric, class]
    mo = np.stack([min_overlaps[:, metric, m] for m in range(len(current_classes)) for _ in difficultys]).reshape(-1)
    cfg_mo = torch.from_numpy(np.ascontiguousarray(mo)).to(dev)
    tp_scores, tp_count = ops.kitti_eval_tp_scores(t["gt_off"], t["dt_off"], t["ov_off"], overlaps, t["dt_score"], ign_gt, ign_dt, p["max_gt"],
                                                   p["max_dt"], cfg_mo, num_k)
    thresholds, n_thr, sorted_scores, n_scores = ops.kitti_eval_thresholds(tp_scores, tp_count, nvg, num_k)
    counts, sim = ops.kitti_eval_pr(t["gt_off"], t["dt_off"], t["dc_off"], t["ov_off"], overlaps, t["dt_score"], t["gt_alpha"], t["dt_alpha"],
                                    t["dt_bbox"], t["dc_bbox"], ign_gt, ign_dt, p["max_gt"], p["max_dt"], cfg_mo, num_k, thresholds, n_thr,
                                    metric, compute_aos)
    out.update(tp_scores=tp_scores, tp_count=tp_count, sorted_scores=sorted_scores, n_scores=n_scores, thresholds=thresholds,
               n_thresholds=n_thr, counts=counts, similarity=sim, cfg_min_overlap=cfg_mo)
    return out


def finish(counts, similarity, thresholds, n_thresholds, shape, compute_aos):
    """The host end of eval_class_v3 (eval.py:581-591) on numpy arrays: precision = tp / (tp + fp) in float64 (0 / 0 is the NaN the
    reference gets), the running maximum from the right (np.max semantics: a NaN spreads to the left), the same for aos; entries
    behind a configuration's threshold count stay zero.  -> (precision, aos, thresholds), each ``shape + (41,)``."""
    configs = counts.shape[0]
    precision = np.zeros((configs, N_SAMPLE_PTS))
    aos = np.zeros((configs, N_SAMPLE_PTS))
    all_thresholds = np.zeros((configs, N_SAMPLE_PTS))
    tp, fp = counts[:, :, 0].astype(np.float64), counts[:, :, 1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(configs):
            n = int(n_thresholds[c])
            all_thresholds[c, :n] = thresholds[c, :n]
            precision[c, :n] = tp[c, :n] / (tp[c, :n] + fp[c, :n])
            if compute_aos:
                aos[c, :n] = similarity[c, :n] / (tp[c, :n] + fp[c, :n])
            # np.max(x[i:]) for every i < n: the tail behind n is zeros and takes part, as in the reference
            for i in range(n):
                precision[c, i] = np.max(precision[c, i:])
                if compute_aos:
                    aos[c, i] = np.max(aos[c, i:])
    return precision.reshape(*shape, N_SAMPLE_PTS), aos.reshape(*shape, N_SAMPLE_PTS), all_thresholds.reshape(*shape, N_SAMPLE_PTS)


def eval_class_v3(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, z_axis=1, z_center=1.0,
                  num_parts=50):
    """Kitti eval, the reference's signature and return dict (``num_parts`` is accepted and ignored: nothing is computed in parts).
    An image above a cap of the device form (ops.KITTI_EVAL_MAX_GT / _MAX_DT): the reference's own function serves the call,
    counted in ``stats['fallback']``."""
    from . import ops
    assert len(gt_annos) == len(dt_annos)
    p = pack(gt_annos, dt_annos)
    if p["max_gt"] > ops.KITTI_EVAL_MAX_GT or p["max_dt"] > ops.KITTI_EVAL_MAX_DT:
        stats["fallback"] += 1
        return _reference_eval_class_v3()(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos, z_axis=z_axis,
                                          z_center=z_center, num_parts=num_parts)
    stats["device"] += 1
    r = run_stages(p, current_classes, difficultys, metric, min_overlaps, compute_aos, z_axis, z_center)
    shape = (len(current_classes), len(difficultys), len(min_overlaps))
    precision, aos, all_thresholds = finish(r["counts"].cpu().numpy(), r["similarity"].cpu().numpy(), r["thresholds"].cpu().numpy(),
                                            r["n_thresholds"].cpu().numpy(), shape, compute_aos)
    return {
        "recall": np.zeros(shape + (N_SAMPLE_PTS,)),          # zeros in the reference too (its recall code is commented out)
        "precision": precision,
        "orientation": aos,
        "thresholds": all_thresholds,
        "min_overlaps": min_overlaps,
    }
