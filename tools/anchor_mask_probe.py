"""Probe: what the anchor-area mask costs and buys at batch 8 of pointpillars/car/xyres_16 (KITTI_PP_CAR_16: 432 x 496 pillars,
107 136 anchors per frame).  Clouds are synthetic (second_amd.synthetic, cropped to the range); medians of three windows of >= 0.5 s
after warm-up.
  (a) the mask chain alone (clear, count, two scans, one thread per anchor) replayed from a hipGraph: microseconds per batch;
  (b) ``compat.accelerate_model`` on the reference-shaped network object (tests/reference_standin.py) with examples that carry
      ``anchors_mask``: frames/s, against the SAME examples with ``anchors_mask`` popped (same build: what the masked select adds)
      and against the module graph of the un-accelerated object (what such examples got before the fused path took them).
    python tools/anchor_mask_probe.py [--out profiles/anchor_mask_probe_pp_car16_bs8.json]            (prints one JSON line)"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "second.pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from second_amd import compat, ops, synthetic as syn  # noqa: E402
from second_amd.models import KITTI_PP_CAR_16 as CFG  # noqa: E402

BATCH, POINTS, PILLARS = 8, 9000, 6000


def windows(step, sync, per_step, seconds=0.5, runs=3, warmup=10):
    """``per_step`` units per second: median of ``runs`` windows of >= ``seconds`` each, after ``warmup`` steps"""
    for _ in range(warmup):
        step()
    sync()
    out = []
    for _ in range(runs):
        n, t0 = 0, time.perf_counter()
        while True:
            step()
            n += 1
            if n % 8 == 0:
                sync()
                if time.perf_counter() - t0 >= seconds:
                    break
        sync()
        out.append(n * per_step / (time.perf_counter() - t0))
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from reference_standin import build_voxelnet, example_of
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    clouds = [syn.syn_kitti_cloud(s, num_points=POINTS, num_voxels=PILLARS, point_cloud_range=tuple(CFG["point_cloud_range"]),
                                  voxel_size=tuple(CFG["voxel_size"])) for s in range(BATCH)]
    torch.manual_seed(0)
    net = build_voxelnet(CFG)
    syn.randomise_like_trained(net, seed=1)
    net = net.eval().to(dev)
    ex = example_of(net, clouds, dev)
    with torch.no_grad():
        one = ex["coordinates"][:, 0] == 0
        p = net.network_forward(ex["voxels"][one], ex["num_points"][one], ex["coordinates"][one], 1)
        syn.sharpen_heads(net, p["cls_preds"].float(), p["box_preds"].float())
    prop = torch.cuda.get_device_properties(dev)
    res = {"network": CFG["name"], "batch": BATCH, "points_per_cloud": POINTS, "pillars_per_cloud": PILLARS, "clouds": "synthetic",
           "anchors_per_frame": int(net.anchors.shape[0]), "anchor_area_threshold": CFG["anchor_area_threshold"],
           "device": torch.cuda.get_device_name(dev), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count}
    # ---- (a) the mask chain alone, from a hipGraph
    vg, gs = net.voxel_generator, net.grid_size
    anchors = net.anchors.to(dev)
    coords = ex["coordinates"].contiguous()
    n_dev = torch.tensor([coords.shape[0]], dtype=torch.int32, device=dev)
    out = torch.zeros((BATCH, anchors.shape[0]), dtype=torch.uint8, device=dev)
    chain = lambda: ops.anchor_area_mask(coords, n_dev, BATCH, (int(gs[1]), int(gs[0])), anchors, vg.voxel_size[:2], vg.point_cloud_range[:2],
                                         CFG["anchor_area_threshold"], out=out)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    per_s, runs = windows(graph.replay, torch.cuda.synchronize, 1.0)
    res["mask_chain"] = {"us_per_batch": round(1e6 / per_s, 2), "runs_us": [round(1e6 / v, 2) for v in runs],
                         "kept_share": round(float(out.float().mean()), 4)}
    ex_mask = dict(ex, anchors_mask=out.clone())
    ex_plain = dict(ex)
    # ---- (b) the module graph (the un-accelerated object; its predict has no mask: what the fused path replaces for these examples)
    with torch.no_grad():
        f, runs = windows(lambda: net(ex_plain), torch.cuda.synchronize, BATCH, warmup=3)
    res["module_graph"] = {"frames_per_s": round(f, 1), "runs": [round(v, 1) for v in runs]}
    # ---- (c) accelerate_model: with the mask, and the same examples with it popped
    compat.accelerate_model(net)
    eng = net._second_amd_engine
    res["fused"] = {}
    with torch.no_grad():
        for label, e in (("with_mask", ex_mask), ("mask_popped", ex_plain)):
            dets = sum(int(r["scores"].shape[0]) for r in net(e))
            f, runs = windows(lambda: net(e), torch.cuda.synchronize, BATCH)
            res["fused"][label] = {"frames_per_s": round(f, 1), "runs": [round(v, 1) for v in runs], "detections": dets}
    res["fused"]["stats"] = {k: v for k, v in eng.stats.items() if isinstance(v, int)}
    res["fused"]["arithmetic"] = eng._det.arithmetic()
    step_us = 1e6 * BATCH / res["fused"]["with_mask"]["frames_per_s"]
    res["mask_select_cost_share"] = round(1.0 - res["fused"]["with_mask"]["frames_per_s"] / res["fused"]["mask_popped"]["frames_per_s"], 4)
    res["mask_chain_share_of_step"] = round(res["mask_chain"]["us_per_batch"] / step_us, 4)
    res["speedup_over_module_graph"] = round(res["fused"]["with_mask"]["frames_per_s"] / res["module_graph"]["frames_per_s"], 2)
    assert eng.stats["original_calls"] == 0, eng.stats
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
