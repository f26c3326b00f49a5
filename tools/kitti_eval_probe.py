"""Probe: one KITTI val pass of AP evaluation -- get_official_eval_result + get_coco_eval_result make six eval_class_v3 calls (bbox,
bev, 3d; official and coco min_overlaps) -- through second_amd.kitti_eval.eval_class_v3 (the sec_kitti_eval_* kernels; host packing,
transfers and the host finish included), and the reference's own eval_class_v3 on a stated subset of the images.

Data: synthetic, seeded -- 3 769 images, Car / Pedestrian / Cyclist, about 6 gt and 10 detections per image (jittered gt, false
positives, DontCare regions).  Device: medians of three passes after a warm-up pass.  Reference: plain Python under the numba stub
(numba is not installed here), ONE run, on the CPU of the machine the probe runs on -- NOT a numba figure; it needs the reference
checkout (SECOND_REFERENCE) and, for metrics 1 / 2, a GPU for the rotated IoU it calls (metric 0 alone without one).

    python tools/kitti_eval_probe.py [--out profiles/kitti_eval_probe.json] [--reference-images 75] [--no-device]   (one JSON line)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "second.pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

IMAGES, CLASSES, CLASS_IDS = 3769, ["Car", "Pedestrian", "Cyclist"], [0, 1, 2]
SIZES = {"Car": (3.9, 1.56, 1.6), "Pedestrian": (0.8, 1.73, 0.6), "Cyclist": (1.76, 1.73, 0.6), "Van": (5.0, 2.1, 1.9), "DontCare": (-1, -1, -1)}


def synthetic_annos(seed=0, images=IMAGES):
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for _ in range(images):
        g = int(rng.poisson(6))
        names = list(rng.choice(["Car", "Pedestrian", "Cyclist", "Van", "DontCare"], g, p=[0.55, 0.15, 0.1, 0.1, 0.1]))
        h = rng.uniform(15, 120, g)
        xy = np.stack([rng.uniform(0, 1100, g), rng.uniform(100, 250, g)], 1)
        gt = dict(name=np.array(names, dtype="U16"), bbox=np.concatenate([xy, xy + np.stack([h * rng.uniform(1, 2.2, g), h], 1)], 1),
                  alpha=rng.uniform(-np.pi, np.pi, g), occluded=rng.choice([0, 0, 1, 2, 3], g).astype(np.int64),
                  truncated=rng.choice([0.0, 0.0, 0.2, 0.4, 0.7], g),
                  location=np.stack([rng.uniform(-25, 25, g), rng.uniform(1.4, 1.9, g), rng.uniform(5, 70, g)], 1),
                  dimensions=np.array([SIZES[n] for n in names]).reshape(g, 3) * rng.uniform(0.9, 1.1, (g, 3)),
                  rotation_y=rng.uniform(-np.pi, np.pi, g))
        d = int(rng.poisson(10))
        src = rng.integers(0, g, d) if g else np.zeros(d, np.int64)
        free = (rng.random(d) < 0.35) | (g == 0)

        def j(k, s):                                              # jittered copies of the gt rows `src`
            base = gt[k][src] if g else np.zeros((d,) + gt[k].shape[1:])
            return base + rng.normal(0, s, base.shape)
        fx = np.stack([rng.uniform(0, 1100, d), rng.uniform(100, 250, d)], 1)
        fbox = np.concatenate([fx, fx + rng.uniform(20, 120, (d, 2))], 1)
        floc = np.stack([rng.uniform(-25, 25, d), rng.uniform(1.4, 1.9, d), rng.uniform(5, 70, d)], 1)
        dnames = [names[s] if (g and not f and names[s] in CLASSES) else str(rng.choice(CLASSES)) for s, f in zip(src, free)]
        dt = dict(name=np.array(dnames, dtype="U16"), bbox=np.where(free[:, None], fbox, j("bbox", 2.0)), alpha=j("alpha", 0.2),
                  score=rng.uniform(0.05, 1.0, d), location=np.where(free[:, None], floc, j("location", 0.1)),
                  dimensions=np.where(free[:, None], np.array([SIZES[n] for n in dnames]).reshape(d, 3), np.abs(j("dimensions", 0.05))),
                  rotation_y=j("rotation_y", 0.1))
        gts.append(gt); dts.append(dt)
    return gts, dts


def min_overlaps(kind):
    if kind == "official":
        return np.array([[[0.7, 0.5, 0.5]] * 3, [[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]]])
    mo = np.zeros((10, 3, 3))
    mo[:, :, 0], mo[:, :, 1:] = np.linspace(0.5, 0.95, 10)[:, None], np.linspace(0.25, 0.7, 10)[:, None, None]
    return mo


def one_pass(fn, gts, dts, metrics):
    """The six calls of get_official_eval_result + get_coco_eval_result (do_eval_v3 / do_eval_v2): aos on every official call and on
    the coco bbox call."""
    out = {}
    for kind in ("official", "coco"):
        for m in metrics:
            out[(kind, m)] = fn(gts, dts, CLASS_IDS, [0, 1, 2], m, min_overlaps(kind), kind == "official" or m == 0, z_axis=1, z_center=1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference-images", type=int, default=75)     # one part of the reference's default partition (3 769 images in 50 parts)
    ap.add_argument("--no-device", action="store_true")
    args = ap.parse_args()
    gts, dts = synthetic_annos()
    res = {"images": IMAGES, "classes": CLASSES, "data": "synthetic", "gt_rows": int(sum(len(g["name"]) for g in gts)),
           "detections": int(sum(len(d["name"]) for d in dts)), "calls_per_pass": 6, "configurations_per_pass": 3 * (18 + 90)}
    if not args.no_device:
        import torch
        from second_amd import kitti_eval as KE
        dev = torch.device("cuda", 0)
        prop = torch.cuda.get_device_properties(dev)
        res.update(device=torch.cuda.get_device_name(dev), arch=getattr(prop, "gcnArchName", ""), compute_units=prop.multi_processor_count)
        last = one_pass(KE.eval_class_v3, gts, dts, range(3))               # warm-up (library load, allocator)
        torch.cuda.synchronize()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            last = one_pass(KE.eval_class_v3, gts, dts, range(3))
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for _ in range(6):
            KE.pack(gts, dts)
        res["device_path"] = {"seconds_per_pass": round(statistics.median(runs), 4), "runs": [round(r, 4) for r in runs],
                              "of_which_host_packing_seconds": round(time.perf_counter() - t0, 4),
                              "car_moderate_bbox_map": round(float(sum(last[("official", 0)]["precision"][0, 1, 0, ::4]) / 11 * 100), 3),
                              "stats": dict(KE.stats)}
    ref_root = os.environ.get("SECOND_REFERENCE", "/root/reference")
    if args.reference_images > 0 and os.path.isdir(os.path.join(ref_root, "second")):
        from second_amd import compat
        compat.install(ref_root)
        ev = compat.accelerate_eval(statistics=False)
        metrics = [0] if args.no_device else [0, 1, 2]
        n = min(args.reference_images, IMAGES)
        t0 = time.perf_counter()
        one_pass(lambda *a, **k: ev.eval_class_v3(*a, num_parts=1, **k), gts[:n], dts[:n], metrics)
        sec = time.perf_counter() - t0
        res["reference_plain_python"] = {"images": n, "metrics": metrics, "seconds": round(sec, 3), "runs": 1,
                                         "seconds_per_image": round(sec / n, 5), "extrapolated_seconds_for_all_images": round(sec / n * IMAGES, 1),
                                         "note": "the reference's eval_class_v3 as plain Python under the numba stub, one run: not a numba figure"}
    else:
        res["reference_plain_python"] = "not measured (no reference checkout on this machine)"
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
