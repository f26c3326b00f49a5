"""Probe: one DeviceDatabaseSampler call at batch 8 on synthetic car.fhd clouds (17 000 points and 5 gt boxes per frame) with a
synthetic pool of 1 000 car-sized objects of 0..400 points (car.fhd.config's sampler: 15 cars, rate 1): eager, its three stages on
their own, ``draw``, and the call replayed from a hipGraph alone and in front of DeviceAugmenter; after warm-up, medians of three
windows of >= 0.5 s.  No KITTI database exists where this runs: every figure is on the synthetic pool.
    python tools/dbsample_probe.py [--out profiles/dbsample_probe_car_fhd_bs8.json]
With ``--reference DIR`` (a checkout of the reference; no GPU needed) it times instead frame 0 of the same batch through the
reference's own DataBaseSamplerV2.sample_all + points_in_rbbox + the concatenations of prep_pointcloud on the CPU, the way they run
in this project's containers: numba's jit stubbed by second_amd.compat, i.e. plain Python -- not a numba figure.  Both modes merge
their keys into ``--out``."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "second.pytorch_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from second_amd import synthetic as syn  # noqa: E402
from augment_probe import CFG, TRIES, windows  # noqa: E402

BATCH, GT_PER_FRAME, POOL, POOL_POINTS, GROUPS = 8, 5, 1000, 400, [("Car", 15)]


def inputs():
    pts, offs = syn.batch_clouds([syn.syn_kitti_cloud(s) for s in range(BATCH)])
    boxes = [syn.syn_kitti_boxes(s, GT_PER_FRAME) for s in range(BATCH)]
    goffs = np.concatenate([[0], np.cumsum([len(b) for b in boxes])]).astype(np.int32)
    return pts, offs, np.concatenate(boxes).astype(np.float32), goffs


def database(device):
    from second_amd.augment import DeviceGtDatabase
    return DeviceGtDatabase.synthetic(0, ("Car",), POOL, max_points=POOL_POINTS, groups=GROUPS, rate=1.0, device=device)


def device_part():
    import torch
    from second_amd import ops, runtime as rt
    from second_amd.augment import DeviceAugmenter, DeviceDatabaseSampler
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pts, offs, gt, goffs = (torch.from_numpy(a).to(dev) for a in inputs())
    classes = torch.ones(gt.shape[0], dtype=torch.int32, device=dev)
    db = database(dev)
    sampler = DeviceDatabaseSampler(db)
    gen = torch.Generator(device=dev).manual_seed(0)
    sampler.draw(gen, batch_size=BATCH)
    sync = torch.cuda.synchronize
    res = {"batch": BATCH, "points": int(pts.shape[0]), "gt_boxes": int(gt.shape[0]), "pool_objects": len(db),
           "pool_points": int(db.pool_points.shape[0]), "groups": GROUPS, "clouds": "synthetic", "pool": "synthetic",
           "device": torch.cuda.get_device_name(dev)}
    args = (pts, offs, gt, goffs, classes)
    out = sampler(*args)
    sel = sampler.last
    res["accepted_per_frame"] = sel["accepted_count"].tolist()
    res["points_out"] = int(out[1][-1].item())
    res["point_capacity"] = int(out[0].shape[0])
    res["overflowed"] = sampler.overflowed()
    res["eager"] = windows(lambda: sampler(*args), sync)
    res["draw"] = windows(lambda: sampler.draw(gen), sync)
    first = ops.points_in_boxes(pts, offs, sel["boxes"], sel["box_offsets"], valid=sel["sampled"])
    res["removed_points"] = int((first >= 0).sum().item())
    buf = torch.zeros_like(out[0])
    res["stage_select_eager"] = windows(lambda: ops.db_sample_select(gt, goffs, classes, db.boxes, sampler.candidates, sampler.class_of_group,
                                                                     sampler.num_table), sync)
    res["stage_points_in_boxes_eager"] = windows(lambda: ops.points_in_boxes(pts, offs, sel["boxes"], sel["box_offsets"], valid=sel["sampled"]), sync)
    res["stage_merge_points_eager"] = windows(lambda: ops.db_sample_merge_points(pts, offs, first, db.pool_points, db.pool_offsets, db.boxes,
                                                                                 sel["accepted"], sel["accepted_count"], out=buf), sync)
    graph = torch.cuda.CUDAGraph()
    with rt.capture_guard(), torch.cuda.graph(graph):
        sampler(*args)
    res["graph_replay"] = windows(graph.replay, sync)
    res["graph_replay"]["us_per_sample"] = round(res["graph_replay"]["us_per_call"] / BATCH, 2)
    aug = DeviceAugmenter(point_cloud_range=syn.CAR_FHD_RANGE, num_try=TRIES, sampler=sampler, **CFG)
    aug.draw(gen, num_boxes=sampler.box_rows(gt.shape[0], BATCH), batch_size=BATCH)
    aug(pts, offs, gt, goffs, classes)
    graph2 = torch.cuda.CUDAGraph()
    with rt.capture_guard(), torch.cuda.graph(graph2):
        both = aug(pts, offs, gt, goffs, classes)
    res["with_augmenter_graph_replay"] = windows(graph2.replay, sync)
    res["with_augmenter_boxes_kept"] = int(both[3][-1].item())
    return res


def reference_part(ref):
    from second_amd import compat
    compat.install(ref)
    from second.core import box_np_ops, preprocess as prep, sample_ops
    pts, offs, gt, goffs = inputs()
    p, b = pts[offs[0]:offs[1]].copy(), gt[goffs[0]:goffs[1]].copy()
    db = database("cpu")
    boxes, pool, po = db.boxes.numpy(), db.pool_points.numpy(), db.pool_offsets.numpy()
    with tempfile.TemporaryDirectory() as root:
        infos = []
        for r in range(len(db)):
            pool[po[r]:po[r + 1]].tofile(os.path.join(root, f"{r}.bin"))
            infos.append(dict(name="Car", path=f"{r}.bin", box3d_lidar=boxes[r].copy(), difficulty=0, num_points_in_gt=int(po[r + 1] - po[r])))
        np.random.seed(0)
        sampler = sample_ops.DataBaseSamplerV2({"Car": infos}, [dict(GROUPS)], None, 1.0, [0.0, 0.0])
        names = np.array(["Car"] * len(b))
        t0 = time.perf_counter()
        ret = sampler.sample_all(root, b, names, p.shape[1])
        t1 = time.perf_counter()
        masks = box_np_ops.points_in_rbbox(p, ret["gt_boxes"])
        merged = np.concatenate([ret["points"], p[np.logical_not(masks.any(-1))]], axis=0)
        t2 = time.perf_counter()
    return {"reference_cpu_plain_python": {"what": "one sample (frame 0 of the batch) through the reference's sample_all and the merge of "
                                                   "prep_pointcloud with numba's jit stubbed (second_amd.compat): plain Python on this CPU, "
                                                   "one run, .bin files read from a temporary directory, not a numba figure",
                                           "points": int(len(p)), "gt_boxes": int(len(b)), "accepted": int(len(ret["gt_boxes"])),
                                           "points_out": int(len(merged)), "removed_points": int(masks.any(-1).sum()),
                                           "sample_all_s": round(t1 - t0, 4), "remove_and_merge_s": round(t2 - t1, 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", default=None, help="time the reference's CPU functions instead (no GPU needed)")
    args = ap.parse_args()
    res = reference_part(args.reference) if args.reference else device_part()
    if args.out and os.path.exists(args.out):
        res = dict(json.load(open(args.out)), **res)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
