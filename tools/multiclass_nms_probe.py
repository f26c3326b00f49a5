"""Probe: multi-class NMS (use_multi_class_nms) on the nuScenes all.fhd head -- ten classes, 20 anchors per cell of a 124 x 124 map
(307 520 anchors per frame), batch 8, bf16 logits, that config's pre 1000 / post 300 / threshold 0.05 / IoU 0.5 for every class.
Head tensors are synthetic (channels-last, a -6 floor with a few hundred elevated logits per frame and class range); every figure is
replayed from a hipGraph, medians of three windows of >= 0.5 s after warm-up, microseconds per batch:
  (1) the fused chain over (frame, class) items: select_classes, decode_classes, nms_sorted_items (two launches), finalize_classes;
  (2) the same result from the per-class loop over the entry points that existed before (select on the strided one-class view, decode,
      NMS, finalize: ten times) -- the yardstick;
  (3) the single-list predict (best class per anchor, one NMS), for scale.
(1) and (2) for the config's anchor ranges and for nms_class_agnostic.
    python tools/multiclass_nms_probe.py [--out profiles/multiclass_nms_probe_nusc_fhd_bs8.json]            (prints one JSON line)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "second.pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from second_amd import models as M, ops  # noqa: E402

BATCH, PER_CLASS = 8, 120          # elevated logits per frame and class


def windows(step, sync, seconds=0.5, runs=3, warmup=10):
    """microseconds per step: median of ``runs`` windows of >= ``seconds`` each, after ``warmup`` steps"""
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
        out.append(1e6 * (time.perf_counter() - t0) / n)
    return round(statistics.median(out), 2), [round(v, 2) for v in out]


def graphed(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.rt.capture_guard(), torch.no_grad(), torch.cuda.graph(g):
        out = fn()
    return g, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = M.ALL_FHD_NUSC
    nc = cfg["num_class"]
    gs = M.grid_size_of(cfg)
    fm = [1, int(gs[1]) // cfg["downsample_factor"], int(gs[0]) // cfg["downsample_factor"]]
    h, w = fm[1], fm[2]
    begin = M.anchor_class_ranges(cfg, fm)
    a = begin[-1] // (h * w)
    rng = np.random.default_rng(0)
    cls = np.full((BATCH, a * h * w, nc), -6.0, np.float32) + rng.normal(0, 0.4, (BATCH, a * h * w, nc)).astype(np.float32)
    for b in range(BATCH):
        for c in range(nc):
            idx = rng.integers(begin[c], begin[c + 1], PER_CLASS)
            cls[b, idx, c] = rng.normal(-0.5, 1.5, PER_CLASS)
    def head(t, code):          # [B, A, H, W, code] view of a channels-last tensor, as the RPN head leaves it
        t = torch.from_numpy(t.reshape(BATCH, a, h, w, code)).to(torch.bfloat16).to(dev)
        return t.permute(0, 2, 3, 1, 4).contiguous().permute(0, 3, 1, 2, 4)
    preds = {"cls_preds": head(cls, nc), "box_preds": head(rng.normal(0, 0.2, (BATCH, a * h * w, 7)).astype(np.float32), 7),
             "dir_cls_preds": head(rng.normal(0, 1, (BATCH, a * h * w, 2)).astype(np.float32), 2)}
    prop = torch.cuda.get_device_properties(dev)
    res = {"network": cfg["name"], "batch": BATCH, "classes": nc, "map": [h, w], "anchors_per_frame": a * h * w, "dtype": "bfloat16",
           "heads": "synthetic", "pre": cfg["nms_pre_max_size"], "post": cfg["nms_post_max_size"], "threshold": cfg["nms_score_threshold"],
           "iou": cfg["nms_iou_threshold"], "device": torch.cuda.get_device_name(dev), "arch": getattr(prop, "gcnArchName", ""),
           "compute_units": prop.multi_processor_count, "unit": "us per batch"}

    def loop(det):
        """the per-class loop over sec_predict_select / _decode / sec_nms_sorted_f32 / sec_predict_finalize"""
        mc, c5, b5, d5 = det.multiclass, preds["cls_preds"], preds["box_preds"], preds["dir_cls_preds"]
        kind, sem = ("rotate", "cpu") if cfg["use_rotate_nms"] else ("axis_aligned", "numba")
        outs = []
        for c, (a0, a1) in enumerate(mc["a_ranges"]):
            idx, score, lab, cnt = ops.predict_select(c5[:, a0:a1, :, :, c:c + 1], mc["pre"][c], mc["thr"][c])
            idx = idx + a0 * h * w                                    # (one torch launch per class: rebasing to the full anchor list)
            dec, dets, dlab = ops.predict_decode(b5, d5, det.anchors, idx, score, rotate=cfg["use_rotate_nms"])
            keep, num = ops.nms_sorted(dets, cnt, mc["iou"][c], kind, sem, post_max=mc["post"][c])
            outs.append(ops.predict_finalize(dec, score, lab, dlab, keep, num, mc["post"][c], True, cfg["direction_offset"],
                                             cfg["direction_limit_offset"], cfg["num_direction_bins"], det.post_center_range))
        return outs

    for mode, agnostic in (("anchor_ranges", False), ("class_agnostic", True)):
        det = M.SecondDetector(dict(cfg, multiclass_nms=True, nms_class_agnostic=agnostic)).eval().to(dev)
        g1, out1 = graphed(lambda: det._predict_multiclass_fused(preds, BATCH, det.anchors))
        g2, out2 = graphed(lambda: loop(det))
        torch.cuda.synchronize()
        # same survivors from both
        off = det.multiclass["post_offsets"]
        for c, o in enumerate(out2):
            seg = slice(off[c], off[c + 1])
            assert torch.equal(out1["valid"][:, seg], o["valid"]) and torch.equal(out1["scores"][:, seg][o["valid"]], o["scores"][o["valid"]]), (mode, c)
        f1, r1 = windows(g1.replay, torch.cuda.synchronize)
        f2, r2 = windows(g2.replay, torch.cuda.synchronize)
        res[mode] = {"fused_chain": f1, "fused_chain_runs": r1, "per_class_loop": f2, "per_class_loop_runs": r2,
                     "fused_over_loop": round(f1 / f2, 4), "detections": int(out1["valid"].sum())}
    single = M.SecondDetector(cfg).eval().to(dev)
    g3, out3 = graphed(lambda: single._predict_fused(preds, BATCH, single.anchors))
    f3, r3 = windows(g3.replay, torch.cuda.synchronize)
    res["single_list_predict"] = {"us": f3, "runs": r3, "detections": int(out3["valid"].sum())}
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
