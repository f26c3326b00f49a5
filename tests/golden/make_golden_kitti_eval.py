"""Produces tests/golden/kitti_eval.npz by EXECUTING the reference's KITTI evaluation on CPU: calculate_iou_partly, clean_data,
compute_statistics_jit, get_thresholds, fused_compute_statistics and eval_class_v3 through get_official_eval_result and
get_coco_eval_result of second/utils/eval.py.  Build container only (needs the reference checkout):

    python tests/golden/make_golden_kitti_eval.py [path to the reference checkout]

numba is stubbed by make_golden.install_shims (as for every other fixture): the jitted loops run as plain Python, rotate_iou_gpu_eval
runs through the SIMT emulator.  Three things are arranged around the reference, neither touches a number it computes:
  * get_split_parts is replaced by "every image is its own part".  With the default num_parts = 50 the reference cannot evaluate
    fewer than 50 images at all (a part of zero images makes np.concatenate fail); the partition only decides which rectangle of the
    overlap matrix is computed before the per-image blocks are cut out, and one image per part keeps the emulator run short;
  * np.linspace takes the float64 count do_coco_style_eval passes (eval.py:704; a TypeError since numpy 1.18);
  * rotate_iou_gpu_eval is memoised on its arguments (the six eval_class_v3 calls of a case ask for the same matrices).
What eval_class_v3 computes on the way is recorded by wrapping get_thresholds and fused_compute_statistics (module globals, resolved
at call time).  The cases are seeded below and reseeded until the reference's own numbers satisfy the condition of the matching tests:
for metrics 1 and 2 no same-image overlap lies within 1e-4 of any min_overlap in use (the smallest distance is recorded).  The layout
of the file is tests/kitti_eval_helpers.py's (store_annos / load_case / recorded), whose numpy restatement is checked against the
recorded arrays here as well -- that is also where the branch counters asserted for case A come from."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SIZES = {"Car": (3.9, 1.56, 1.6), "Van": (5.0, 2.1, 1.9), "Pedestrian": (0.8, 1.73, 0.6), "Person_sitting": (0.8, 1.2, 0.6),
         "Cyclist": (1.76, 1.73, 0.6), "DontCare": (-1.0, -1.0, -1.0), "car": (4.6, 1.9, 1.7)}        # (l, h, w)
HEIGHTS = [18.0, 24.0, 25.0, 26.0, 33.0, 39.0, 40.0, 41.0, 55.0, 80.0]                                   # bbox heights straddling 25 and 40 px


def make_gt(rng, names, lidar):
    n = len(names)
    size = np.array([SIZES[x] for x in names]).reshape(n, 3) * rng.uniform(0.9, 1.1, (n, 3))
    if lidar:      # (x, y, z) with z up, dimensions (w, l, h), box centre at z + h / 2 (z_center 0.5)
        loc = np.stack([rng.uniform(5, 60, n), rng.uniform(-20, 20, n), rng.uniform(-1.2, -0.6, n)], 1)
        dims = size[:, [2, 0, 1]]
    else:          # camera: y down, dimensions (l, h, w), box bottom at y (z_center 1.0)
        loc = np.stack([rng.uniform(-20, 20, n), rng.uniform(1.4, 1.9, n), rng.uniform(5, 60, n)], 1)
        dims = size
    h = rng.choice(HEIGHTS, n)
    xy = np.stack([rng.uniform(0, 1100, n), rng.uniform(100, 280, n)], 1)
    bbox = np.concatenate([xy, xy + np.stack([h * rng.uniform(1.0, 2.2, n), h], 1)], 1)
    return dict(name=np.array(names, dtype="U16"), bbox=bbox, alpha=rng.uniform(-np.pi, np.pi, n),
                occluded=rng.choice([0, 0, 0, 1, 1, 2, 3], n).astype(np.int64), truncated=rng.choice([0.0, 0.0, 0.1, 0.2, 0.4, 0.6], n),
                location=loc, dimensions=dims, rotation_y=rng.uniform(-np.pi, np.pi, n))


def make_dt(rng, gt, det_names, extra, small, in_dontcare, lidar, alpha_valid, tight):
    """Detections of one image: a jittered copy of most gt rows that carry a detectable name, ``extra`` free false positives, ``small``
    copies with a bbox under 25 px placed BEFORE the others, ``in_dontcare`` boxes inside DontCare regions.  Shuffled, except that the
    small copies keep a lower index than the proper detection of the same object."""
    rows = []
    cand = [i for i, n in enumerate(gt["name"]) if n in det_names or n in ("Van", "Person_sitting")]
    dc = [i for i, n in enumerate(gt["name"]) if n == "DontCare"]

    def copy_of(i, name, jitter, px):
        b = gt["bbox"][i] + rng.normal(0, px, 4)
        return dict(name=name, bbox=b, alpha=gt["alpha"][i] + rng.normal(0, 0.2), location=gt["location"][i] + rng.normal(0, jitter, 3),
                    dimensions=gt["dimensions"][i] * rng.uniform(1 - jitter / 2, 1 + jitter / 2, 3), rotation_y=gt["rotation_y"][i] + rng.normal(0, jitter))
    for i in cand:
        if rng.random() < (0.0 if tight else 0.12):
            continue                                                   # a missed object
        name = gt["name"][i] if gt["name"][i] in det_names else det_names[0]
        j = 0.03 if (tight or rng.random() < 0.6) else rng.choice([0.1, 0.25])
        rows.append(copy_of(i, name, j, 0.8 if j == 0.03 else 3.0))
    order = list(rng.permutation(len(rows)))
    rows = [rows[k] for k in order]
    people = [i for i in cand if gt["name"][i] != "Car"] if not lidar else cand          # case A: every valid Car keeps its detection, recall 1
    for i in list(rng.choice(people, min(small, len(people)), replace=False)) if people and small else []:
        r = copy_of(i, gt["name"][i] if gt["name"][i] in det_names else det_names[0], 0.05, 1.0)
        r["bbox"][3] = r["bbox"][1] + rng.choice([12.0, 20.0, 24.0])   # under 25 px: ignored_det = 1 at every difficulty
        rows.insert(int(rng.integers(0, max(len(rows) // 3, 1))), r)
    for _ in range(extra):
        g = make_gt(rng, [str(rng.choice(det_names))], lidar)
        rows.insert(int(rng.integers(0, len(rows) + 1)), {k: g[k][0] for k in ("name", "bbox", "alpha", "location", "dimensions", "rotation_y")})
    for i in list(rng.choice(dc, min(in_dontcare, len(dc)), replace=False)) if dc and in_dontcare else []:
        g = make_gt(rng, [str(rng.choice(det_names))], lidar)
        x0, y0, x1, y1 = gt["bbox"][i]
        w, h = (x1 - x0) * rng.uniform(0.5, 0.9), max((y1 - y0) * rng.uniform(0.7, 0.95), 26.0)
        r = {k: g[k][0] for k in ("name", "bbox", "alpha", "location", "dimensions", "rotation_y")}
        r["bbox"] = np.array([x0 + 1, y0 + 1, x0 + 1 + w, y0 + 1 + min(h, y1 - y0 - 1.5)])
        rows.insert(int(rng.integers(0, len(rows) + 1)), r)
    n = len(rows)
    score = np.round(rng.uniform(0.05, 1.0, n), 3)
    if n >= 4:
        score[rng.choice(n, n // 3, replace=False)] = rng.choice([0.3, 0.5, 0.75], n // 3)     # equal scores within an image
    out = {k: (np.stack([r[k] for r in rows]) if n else np.zeros((0,) + {"bbox": (4,), "location": (3,), "dimensions": (3,)}.get(k, ())))
           for k in ("bbox", "alpha", "location", "dimensions", "rotation_y")}
    out["name"] = np.array([r["name"] for r in rows], dtype="U16")
    out["score"] = score
    if not alpha_valid:
        out["alpha"] = np.full(n, -10.0)
    return out


def case_A(seed):
    rng = np.random.default_rng(seed)
    cars = lambda k: ["Car"] * k
    frames = [cars(18) + ["Pedestrian"] * 3 + ["Cyclist"] * 2 + ["Van", "Person_sitting", "DontCare", "DontCare"],
              cars(17) + ["Pedestrian"] * 2 + ["Cyclist"] * 2 + ["Van", "DontCare"],
              None,                                                       # no gt, a few detections
              cars(18) + ["Pedestrian"] * 4 + ["Cyclist"] + ["Van", "Van", "DontCare", "DontCare", "DontCare"],
              ["Pedestrian"] * 2 + ["Cyclist"] * 2 + ["Person_sitting", "DontCare"],      # gt, no detections (and no Car: Car recall can reach 1)
              cars(16) + ["Pedestrian"] * 3 + ["Cyclist"] * 3 + ["Person_sitting", "DontCare"],
              None,                                                       # neither
              cars(15) + ["Pedestrian"] * 2 + ["Cyclist"] * 2 + ["Van", "DontCare", "DontCare"]]
    det = ["Car", "Pedestrian", "Cyclist"]
    gts, dts = [], []
    for f, names in enumerate(frames):
        names = list(rng.permutation(names)) if names else []
        gt = make_gt(rng, names, False)
        if names:
            gt["occluded"][np.array(names) == "Car"] = rng.choice([0, 0, 1, 2], int((np.array(names) == "Car").sum()))
            gt["truncated"][np.array(names) == "Car"] = rng.choice([0.0, 0.1, 0.2, 0.4], int((np.array(names) == "Car").sum()))
            h = gt["bbox"][:, 3] - gt["bbox"][:, 1]
            near = (np.array(names) == "Car") & (np.abs(h - 25.5) < 1.0)        # a Car of 25 or 26 px: its jittered copy could fall under 25 px
            gt["bbox"][near, 3] += 8.0
        if f == 2:
            dt = make_dt(rng, gt, det, 3, 0, 0, False, True, False)
        elif f in (4, 6):
            dt = make_dt(rng, make_gt(rng, [], False), det, 0, 0, 0, False, True, False)
        else:
            dt = make_dt(rng, gt, det, 3, 2, 2, False, True, tight=True)
        gts.append(gt); dts.append(dt)
    return gts, dts


def case_B(seed):
    rng = np.random.default_rng(seed)
    counts = [(6, 0), (9, 0), (22, 45), (0, 0), (7, 0)]          # (gt, free false positives): image 2 ends with 70 detections
    gts, dts = [], []
    for g, extra in counts:
        gt = make_gt(rng, ["car"] * g, True)
        dt = make_dt(rng, gt, ["car"], extra if extra else 2, 1 if g else 0, 0, True, False, False)
        if extra:
            while len(dt["name"]) != 70:
                dt = make_dt(rng, gt, ["car"], extra + 70 - len(dt["name"]), 1, 0, True, False, False)
        gts.append(gt); dts.append(dt)
    return gts, dts


def main():
    if len(sys.argv) > 1:
        os.environ["SECOND_REFERENCE"] = sys.argv[1]
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import make_golden
    make_golden.install_shims()
    import kitti_eval_helpers as H
    import second.utils.eval as ev

    ev.get_split_parts = lambda num, num_part: [1] * num
    _linspace = np.linspace
    np.linspace = lambda start, stop, num=50, *a, **k: _linspace(start, stop, int(num), *a, **k)      # eval.py:704 passes a float64 count
    memo, raw_iou = {}, ev.rotate_iou_gpu_eval

    def iou_memo(boxes, query_boxes, criterion=-1, device_id=0):
        key = (np.asarray(boxes).tobytes(), np.asarray(query_boxes).tobytes(), int(criterion))
        if key not in memo:
            memo[key] = raw_iou(boxes, query_boxes, criterion, device_id)
        return memo[key].copy()
    ev.rotate_iou_gpu_eval = iou_memo

    rec = {"cur": None}
    raw_thr, raw_fused, raw_v3 = ev.get_thresholds, ev.fused_compute_statistics, ev.eval_class_v3

    def thr_wrap(scores, num_gt, num_sample_pts=41):
        rec["cur"]["scores"].append(np.sort(np.asarray(scores, np.float64))[::-1].copy())
        th = raw_thr(scores, num_gt, num_sample_pts)
        rec["cur"]["thresholds"].append(np.array(th, np.float64))
        return th

    def fused_wrap(overlaps, pr, *a, **k):
        if not rec["cur"]["pr"] or rec["cur"]["pr"][-1] is not pr:
            rec["cur"]["pr"].append(pr)                                  # one array per configuration, filled part by part
        return raw_fused(overlaps, pr, *a, **k)
    ev.get_thresholds, ev.fused_compute_statistics = thr_wrap, fused_wrap
    calls = {}

    def v3_wrap(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, **kw):
        rec["cur"] = dict(scores=[], thresholds=[], pr=[])
        ret = raw_v3(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos, **kw)
        calls[(rec["kind"], metric)] = dict(rec["cur"], ret=ret, compute_aos=bool(compute_aos), min_overlaps=np.array(min_overlaps))
        return ret
    ev.eval_class_v3 = v3_wrap

    out = {}
    for name, case in H.CASES.items():
        seed = {"A": 100, "B": 200}[name]
        while True:
            gts, dts = (case_A if name == "A" else case_B)(seed)
            n_img = len(gts)
            assert n_img == case["images"]
            ov = {m: ev.calculate_iou_partly(dts, gts, m, n_img, z_axis=case["z_axis"], z_center=case["z_center"])[0] for m in range(3)}
            in_use = np.unique(np.concatenate([H.min_overlaps_of(k, case["class_ids"])[:, 1:].reshape(-1) for k in H.KINDS]))
            vals = np.concatenate([o.reshape(-1) for m in (1, 2) for o in ov[m]])
            dist = float(np.abs(vals[:, None] - in_use[None, :]).min()) if len(vals) else 1.0
            print(name, "seed", seed, "gt", [len(g["name"]) for g in gts], "dt", [len(d["name"]) for d in dts], "min distance to a threshold", dist)
            if dist > 1e-4:
                break
            seed += 1
        out[f"{name}_seed"], out[f"{name}_min_distance"] = np.int64(seed), np.float64(dist)
        H.store_annos(out, f"{name}_gt", gts, H.GT_KEYS)
        H.store_annos(out, f"{name}_dt", dts, H.DT_KEYS)
        for m in range(3):
            for o, g, d in zip(ov[m], gts, dts):
                assert o.shape == (len(d["name"]), len(g["name"])) and o.dtype == np.float64       # detection-major
            out[f"{name}_overlaps_m{m}"] = np.concatenate([o.reshape(-1) for o in ov[m]]) if n_img else np.zeros(0)
        assert all(float(np.float32(v)) == v for v in out[f"{name}_overlaps_m2"])                  # metric 2 went through a float32 array
        ig, idt, nvg = [], [], []
        for c in case["class_ids"]:
            for d in H.DIFFICULTYS:
                r = [ev.clean_data(g, t, c, d) for g, t in zip(gts, dts)]
                ig.append(np.concatenate([np.array(x[1], np.int8) for x in r])); idt.append(np.concatenate([np.array(x[2], np.int8) for x in r]))
                nvg.append(sum(x[0] for x in r))
        out[f"{name}_ignored_gt"], out[f"{name}_ignored_dt"], out[f"{name}_num_valid_gt"] = np.stack(ig), np.stack(idt), np.array(nvg, np.int32)
        rec["kind"] = "official"
        res = {"official": ev.get_official_eval_result(gts, dts, case["classes"], z_axis=case["z_axis"], z_center=case["z_center"])}
        rec["kind"] = "coco"
        res["coco"] = ev.get_coco_eval_result(gts, dts, case["classes"], z_axis=case["z_axis"], z_center=case["z_center"])
        counters = {}
        n_thr_all = []
        for kind in H.KINDS:
            out[f"{name}_{kind}_result"] = np.array(res[kind]["result"])
            out[f"{name}_{kind}_detail"] = np.array(json.dumps(res[kind]["detail"]))
            print(res[kind]["result"])
            for m in range(3):
                c = calls[(kind, m)]
                mo = H.min_overlaps_of(kind, case["class_ids"])
                assert np.array_equal(mo, c["min_overlaps"]), "kitti_eval_helpers.min_overlaps_of is not the reference's table"
                assert c["compute_aos"] == (case["compute_aos"] and (kind == "official" or m == 0))
                configs = len(c["scores"])
                assert configs == len(case["class_ids"]) * 3 * mo.shape[0] == len(c["pr"]) == len(c["thresholds"])
                p = f"{name}_{kind}_m{m}_"
                out[p + "compute_aos"] = np.bool_(c["compute_aos"])
                out[p + "n_scores"] = np.array([len(s) for s in c["scores"]], np.int32)
                out[p + "scores"] = np.concatenate(c["scores"]) if configs else np.zeros(0)
                thr, pr = np.zeros((configs, 41)), np.zeros((configs, 41, 4))
                for i in range(configs):
                    n = len(c["thresholds"][i])
                    assert n <= 41 and c["pr"][i].shape == (n, 4)
                    thr[i, :n], pr[i, :n] = c["thresholds"][i], c["pr"][i]
                out[p + "thresholds"], out[p + "pr"] = thr, pr
                out[p + "n_thresholds"] = np.array([len(t) for t in c["thresholds"]], np.int32)
                out[p + "precision"], out[p + "orientation"] = c["ret"]["precision"], c["ret"]["orientation"]
                assert not c["ret"]["recall"].any() and np.array_equal(c["ret"]["thresholds"].reshape(configs, 41), thr)
                n_thr_all += [len(t) for t in c["thresholds"]]
                # the restatement the GPU tests lean on, against what was just recorded
                mine = H.eval_np(gts, dts, ov[m], case["class_ids"], H.DIFFICULTYS, m, mo, c["compute_aos"], counters)
                assert np.array_equal(mine["ignored_gt"], out[f"{name}_ignored_gt"]) and np.array_equal(mine["ignored_dt"], out[f"{name}_ignored_dt"])
                assert np.array_equal(mine["num_valid_gt"], out[f"{name}_num_valid_gt"])
                assert all(np.array_equal(a, b) for a, b in zip(mine["scores"], c["scores"]))
                assert np.array_equal(mine["thresholds"], thr) and np.array_equal(mine["pr"][..., :3], pr[..., :3])
                assert (np.abs(mine["pr"][..., 3] - pr[..., 3]) <= H.similarity_bound(pr)).all()
                assert np.array_equal(mine["precision"], c["ret"]["precision"], equal_nan=True)
        print(name, "threshold counts: min", min(n_thr_all), "max", max(n_thr_all), "counters", counters)
        if name == "A":
            assert max(n_thr_all) == 41 and min(n_thr_all) < 5
            assert counters.get("nstuff", 0) > 0 and counters.get("replaced_ignored_det", 0) > 0
    path = os.path.join(HERE, "kitti_eval.npz")
    H.save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
