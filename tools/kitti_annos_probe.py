"""Probe: the step between the detector and the AP evaluation of one KITTI val pass -- detections -> KITTI annotation dicts -> what
``kitti_eval.run_stages`` wants on the device -- three ways:

  host     the per-image conversion as the float64 numpy restatement of KittiDataset.convert_detection_to_kitti_annos
           (tests/kitti_annos_helpers.py: vectorised over an image's detections like the reference's numpy calls, error bounds
           included, the reference's per-detection append loop and its three device->host copies NOT included), detections already
           on the host; and, where the reference checkout is present (SECOND_REFERENCE), the reference's own method on CPU tensors,
           one run;
  device   second_amd.kitti_annos.convert_detection_to_kitti_annos: concatenation on the device, the three launches of
           sec_kitti_annos_f64, ONE device->host copy, the dicts built as views;
  pack     the six ``kitti_eval.pack`` calls of a val pass plus the uploads ``run_stages`` makes of their results, for the same
           annotations as a plain list (today's route) and as the DeviceAnnoList hand-off (gt side packed and uploaded once).

Data: synthetic, seeded -- 3 769 images with tools/kitti_eval_probe.py's counts (gt Poisson(6), detections Poisson(10)), KITTI-like
calibrations.  Medians of three windows after a warm-up.  Without a GPU (``--no-device``) only the host figure is measured and the
others read "not measured".

    python tools/kitti_annos_probe.py [--out profiles/kitti_annos_probe.json] [--no-device]   (one JSON line)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "second.pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

IMAGES, CLASSES = 3769, ["Car", "Pedestrian", "Cyclist"]
NOT_MEASURED = "not measured"


def median3(fn, sync=None):
    fn()
    runs = []
    for _ in range(3):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        runs.append(time.perf_counter() - t0)
    return round(statistics.median(runs), 5), [round(r, 5) for r in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-device", action="store_true")
    args = ap.parse_args()
    import kitti_annos_helpers as H
    import kitti_eval_probe as EP
    rng = np.random.default_rng(0)
    counts = rng.poisson(10, IMAGES)
    det_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    n = int(det_off[-1])
    rect, trv2c, p2, shape = H.synthetic_calibration(rng, IMAGES)
    boxes = H.random_boxes(rng, n)
    boxes[:, 0], boxes[:, 1] = rng.uniform(2, 70, n), rng.uniform(-25, 25, n)            # mostly in front of the camera, as after NMS
    scores, labels = rng.uniform(0.05, 1, n).astype(np.float32), rng.integers(0, 3, n).astype(np.int64)
    infos = [{"image": {"image_idx": i, "image_shape": shape[i]}, "calib": {"R0_rect": rect[i], "Tr_velo_to_cam": trv2c[i], "P2": p2[i]}} for i in range(IMAGES)]
    gts, _ = EP.synthetic_annos(images=IMAGES)
    res = {"images": IMAGES, "detections": n, "classes": CLASSES, "data": "synthetic", "windows": 3}

    def host_route():
        kept = 0
        for i in range(IMAGES):
            a, b = det_off[i], det_off[i + 1]
            r = H.restate(boxes[a:b], [0, b - a], (rect[i] @ trv2c[i])[None], p2[i][None], shape[i][None])
            kept += int(r["keep"].sum())
        return kept
    sec, runs = median3(host_route)
    res["host_restatement"] = {"seconds_per_pass": sec, "runs": runs, "microseconds_per_image": round(sec / IMAGES * 1e6, 1), "kept": host_route(),
                               "note": "numpy restatement per image incl. its error bounds, without the reference's per-detection append loop"}
    ref_root = os.environ.get("SECOND_REFERENCE", "/root/reference")
    if os.path.isdir(os.path.join(ref_root, "second")):
        import torch
        from second_amd import compat
        compat.install(ref_root)
        import importlib
        cls = importlib.import_module("second.data.kitti_dataset").KittiDataset
        method = getattr(cls, "_second_amd_original_convert_detection_to_kitti_annos", cls.convert_detection_to_kitti_annos)
        cpu = [{"box3d_lidar": torch.from_numpy(boxes[det_off[i]:det_off[i + 1]].copy()), "scores": torch.from_numpy(scores[det_off[i]:det_off[i + 1]].copy()),
                "label_preds": torch.from_numpy(labels[det_off[i]:det_off[i + 1]].copy()), "metadata": {"image_idx": i}} for i in range(IMAGES)]
        t0 = time.perf_counter()
        ref = method(H.StandinDataset(infos, CLASSES), cpu)
        res["reference_method_cpu_tensors"] = {"seconds_per_pass": round(time.perf_counter() - t0, 4), "runs": 1, "kept": int(sum(len(a["name"]) for a in ref)),
                                               "note": "the reference's own method on CPU tensors (no device->host copies), on the CPU of this machine"}
    else:
        res["reference_method_cpu_tensors"] = "not measured (no reference checkout on this machine)"
    if args.no_device:
        res.update(device=NOT_MEASURED, device_conversion=NOT_MEASURED, pack_and_upload=NOT_MEASURED)
    else:
        import torch
        from second_amd import kitti_annos as KA, kitti_eval as KE
        dev = torch.device("cuda", 0)
        prop = torch.cuda.get_device_properties(dev)
        res.update(device=torch.cuda.get_device_name(dev), arch=getattr(prop, "gcnArchName", ""), compute_units=prop.multi_processor_count)
        det = [{"box3d_lidar": torch.from_numpy(boxes[det_off[i]:det_off[i + 1]]).to(dev), "scores": torch.from_numpy(scores[det_off[i]:det_off[i + 1]]).to(dev),
                "label_preds": torch.from_numpy(labels[det_off[i]:det_off[i + 1]]).to(dev), "metadata": {"image_idx": i}} for i in range(IMAGES)]
        ds = H.StandinDataset(infos, CLASSES)
        sync = torch.cuda.synchronize
        sec, runs = median3(lambda: KA.convert_detection_to_kitti_annos(ds, det), sync)
        annos = KA.convert_detection_to_kitti_annos(ds, det)
        res["device_conversion"] = {"seconds_per_pass": sec, "runs": runs, "kept": int(sum(len(a["name"]) for a in annos)), "stats": dict(KA.stats),
                                    "note": "device concatenation, three launches, one device->host copy, dict building"}

        def upload(p):
            held = p.get("_device")
            t = {k: torch.from_numpy(v).to(dev) for k, v in p.items() if isinstance(v, np.ndarray) and (held is None or k not in held)}
            if held is not None:
                held.update(t)
            return t

        def six(dts):
            if hasattr(dts, "pack_cache"):
                dts.pack_cache = None                                         # a new val pass packs its gt once
            for _ in range(6):
                upload(KE.pack(gts, dts))
        plain = list(annos)
        sec_plain, runs_plain = median3(lambda: six(plain), sync)
        sec_hand, runs_hand = median3(lambda: six(annos), sync)
        res["pack_and_upload"] = {"calls_per_pass": 6, "plain_list_seconds_per_pass": sec_plain, "plain_list_runs": runs_plain,
                                  "handoff_seconds_per_pass": sec_hand, "handoff_runs": runs_hand}
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
