#!/usr/bin/env python3
"""Side measurement: the target assignment ALONE on the nuScenes all.fhd geometry (124 x 124 feature map, ten anchor groups,
assign_per_class), batch 4, 40 synthetic ground-truth boxes per frame spread over all classes, replayed from a hipGraph.

Two variants, timed alternately in windows of at least 0.5 s; the median of three windows each is reported:
  nearest_iou   every range by near-box IoU through the entry point that knows nothing else (ops.assign_targets_per_class without
                ``similarities``: what the stock ALL_FHD_NUSC trains with)
  config        models.NUSC_FHD_GROUP_SIMILARITY (pedestrian, traffic_cone: distance 1.414) through sec_assign_targets_sim_f32

Needs an MI355X; there is no CPU path.  Writes profiles/assign_probe_nusc_fhd_bs4.json (or the path given as first argument).
Not a bench line and no rate is required of it: it says what the per-range similarity costs."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "second.pytorch_amd")); sys.path.insert(0, ROOT)
import numpy as np
import torch
from second_amd import models, ops

BATCH, BOXES, WINDOW_S, WINDOWS = 4, 40, 0.5, 3


def ground_truth(anchors, begin, rng):
    """BOXES jittered anchors per frame, classes round-robin over the ten groups."""
    gts, cls = [], []
    for _ in range(BATCH):
        c = (np.arange(BOXES) % (len(begin) - 1)) + 1
        b = np.stack([anchors[rng.integers(begin[k - 1], begin[k])] for k in c]).astype(np.float32)
        b[:, :2] += rng.normal(0, 0.3, (BOXES, 2)).astype(np.float32)
        b[:, 3:6] *= rng.uniform(0.9, 1.1, (BOXES, 3)).astype(np.float32)
        b[:, 6] += rng.normal(0, 0.2, BOXES).astype(np.float32)
        order = rng.permutation(BOXES)
        gts.append(b[order]); cls.append(c[order].astype(np.int32))
    return np.concatenate(gts), np.concatenate(cls), (np.arange(BATCH + 1) * BOXES).astype(np.int32)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("assign_probe: needs a GPU (no CPU path)")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "assign_probe_nusc_fhd_bs4.json")
    cfg = models.ALL_FHD_NUSC
    grid = models.grid_size_of(cfg)
    fm = [1, int(grid[1]) // cfg["downsample_factor"], int(grid[0]) // cfg["downsample_factor"]]
    assert fm == [1, 124, 124], fm
    anchors_np = np.asarray(models.generate_anchors(cfg, fm), np.float32).reshape(-1, 7)
    begin = models.anchor_class_ranges(cfg, fm)
    gt, cls, offs = ground_truth(anchors_np, begin, np.random.default_rng(0))
    dev = torch.device("cuda", 0)
    anchors, gt, cls, offs = (torch.from_numpy(a).to(dev) for a in (anchors_np, gt, cls, offs))
    args = (anchors, gt, offs, cls, begin, cfg["group_class_ids"], cfg["matched_thresholds"], cfg["unmatched_thresholds"])
    variants = {"nearest_iou": None, "config": models.NUSC_FHD_GROUP_SIMILARITY}
    graphs, results = {}, {}
    for name, sims in variants.items():
        kw = {} if sims is None else dict(similarities=sims)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                eager = ops.assign_targets_per_class(*args, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with ops.rt.capture_guard(), torch.cuda.graph(g, capture_error_mode="thread_local"):
            out = ops.assign_targets_per_class(*args, **kw)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager)), f"{name}: the replay differs from the eager call"
        graphs[name] = g
        results[name] = dict(positives=int((out[0] > 0).sum().item()), dont_care=int((out[0] < 0).sum().item()), windows_ms=[])
    for _ in range(WINDOWS):                       # alternate the variants: other work shares the machine
        for name, g in graphs.items():
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(200):
                    g.replay()
                torch.cuda.synchronize()
                n += 200
                dt = time.perf_counter() - t0
                if dt >= WINDOW_S:
                    break
            results[name]["windows_ms"].append(dt / n * 1e3)
    for r in results.values():
        r["median_ms"] = float(np.median(r["windows_ms"]))
    record = dict(probe="assign_probe", config=cfg["name"], feature_map=fm, anchors=int(anchors.shape[0]), groups=len(begin) - 1,
                  batch=BATCH, boxes_per_frame=BOXES, window_s=WINDOW_S, windows=WINDOWS, device=torch.cuda.get_device_name(0),
                  what="target assignment alone, one hipGraph replay per call, host clock around replays ending in a synchronise",
                  variants=results)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record))


if __name__ == "__main__":
    main()
