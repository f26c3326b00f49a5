"""Probe: one training iteration of nuscenes/all.pp.mhead at the config's full geometry (400 x 400 pillars, 324 800 anchors), batch 4,
synthetic clouds of 60 000 points, 40 boxes per frame spread over both heads' classes:
  (a) the stand-in's own iteration (tests/reference_standin_mhead.py): module graph in train(), ``loss.backward()``,
      ``clip_grad_norm_``, torch AdamW -- the only way this network trained before, so this is the yardstick (targets are assigned
      once outside the loop, as the reference's data loader does it on the host);
  (b) ``training.MultiHeadDeviceTrainer`` in fp32 and (c) in bf16: voxelisation and target assignment included;
  (d) the PillarFeatureNetRadius layer alone at 4 x 30 000 pillars x 60 slots: forward + backward of the torch formulation against
      sec_pfn_kind_train_fwd / _bwd (SEC_PFN_RADIUS), with the peak memory of each (torch.cuda.max_memory_allocated above the resident inputs);
  (e) the 64-channel 3x3 convolutions that stay on torch in (c) -- block 0 and the small head's tower -- forward + backward alone,
      and their share of the bf16 step (the follow-up DESIGN.md section 9h names).
Medians of three windows of >= 0.5 s after warm-up.  No figure here is a pass criterion.
    python tools/mhead_train_probe.py [--out profiles/mhead_train_probe_bs4.json]            (prints one JSON line)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "second.pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from second_amd import models, ops, synthetic as syn  # noqa: E402
from second_amd.models import ALL_PP_MHEAD, SecondDetector  # noqa: E402
from second_amd.training import MultiHeadDeviceTrainer  # noqa: E402

BATCH, POINTS, BOXES = 4, 60000, 40


def runs_of(step, seconds=0.5, runs=3, warmup=3):
    """iterations/s: medians of ``runs`` windows of >= ``seconds`` each (a device sync every iteration: an iteration is tens of ms)"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        n, t0 = 0, time.perf_counter()
        while True:
            step()
            n += 1
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
        out.append(n / (time.perf_counter() - t0))
    med = statistics.median(out)
    return {"ms_per_iteration": round(1e3 / med, 2), "frames_per_s": round(med * BATCH, 1), "runs_ms": [round(1e3 / v, 2) for v in out]}


def boxes_of(cfg, anchors, seed):
    """BOXES boxes per frame, classes cycling over all ten: an anchor of the class inside +-38 m, nudged."""
    rng = np.random.default_rng(seed)
    begin = models.anchor_class_ranges(cfg, [int(v) for v in cfg["heads"][0]["feature_map_size"]])
    gts, goffs, gcls = [], [0], []
    for _ in range(BATCH):
        cls = np.arange(BOXES) % 10 + 1
        rows = []
        for c in cls:
            seg = anchors[begin[c - 1]:begin[c]]
            seg = seg[(np.abs(seg[:, 0]) < 38) & (np.abs(seg[:, 1]) < 38)]
            rows.append(seg[rng.integers(len(seg))])
        b = np.stack(rows).astype(np.float32)
        b[:, :2] += rng.normal(0, 0.05, (BOXES, 2)).astype(np.float32)
        gts.append(b)
        goffs.append(goffs[-1] + BOXES)
        gcls.append(cls.astype(np.int32))
    return np.concatenate(gts), np.array(goffs, np.int32), np.concatenate(gcls)


def pfn_alone(dev):
    """(d): 4 x 30 000 pillars x 60 slots through the layer, torch formulation vs kernels."""
    from mhead_train_helpers import ragged_pillars
    p, t = BATCH * ALL_PP_MHEAD["max_voxels"], ALL_PP_MHEAD["max_points_per_voxel"]
    vox, num, coors = (v.to(dev) for v in ragged_pillars(p, t, seed=7))
    w = torch.randn(p, 64, device=dev)
    res = {"pillars": p, "slots": t, "channels": 64}
    for backend in ("torch", "hip"):
        torch.manual_seed(0)
        net = models.PillarFeatureNetRadius(4, (64,), ALL_PP_MHEAD["voxel_size"], ALL_PP_MHEAD["point_cloud_range"]).to(dev).train()
        net.train_backend = backend

        def step():
            out = net(vox, num, coors)
            (out * w).sum().backward()
            for q in net.parameters():
                q.grad = None
        step()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        r = runs_of(step)
        res[backend] = {"fwd_bwd_ms": r["ms_per_iteration"], "runs_ms": r["runs_ms"], "peak_mib_above_inputs": round(peak / 2 ** 20, 1)}
        del net
        torch.cuda.empty_cache()
    res["speedup"] = round(res["torch"]["fwd_bwd_ms"] / res["hip"]["fwd_bwd_ms"], 2)
    return res


def conv64_alone(det, dtype, step_ms):
    """The layers that stay on torch because ops.conv2d_wgrad_supported has no 64-channel 3x3 form -- block 0 (400 -> 200) and the
    small head's tower (160 x 160) -- forward + backward alone, through the same models._mixed_block, and their share of the step."""
    dev = next(det.parameters()).device
    res = {}
    for name, blk, side in (("block0", det.rpn.blocks[0], 400), ("tower", det.small_head.net, 160)):
        x = torch.randn(BATCH, 64, side, side, device=dev).to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_()

        def step():
            y = models._mixed_block(blk, x, dtype, True)
            y.float().square().mean().backward()
            x.grad = None
            for q in blk.parameters():
                q.grad = None
        res[name + "_fwd_bwd_ms"] = runs_of(step)["ms_per_iteration"]
    res["share_of_step"] = round((res["block0_fwd_bwd_ms"] + res["tower_fwd_bwd_ms"]) / step_ms, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mhead_helpers import standin
    from reference_standin import example_of
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = ALL_PP_MHEAD
    clouds = [syn.syn_nusc_cloud(s, num_points=POINTS, point_cloud_range=tuple(cfg["point_cloud_range"])) for s in range(BATCH)]
    pts, offs = syn.batch_clouds(clouds)
    prop = torch.cuda.get_device_properties(dev)
    res = {"network": "nuscenes/all.pp.mhead", "batch": BATCH, "points_per_cloud": POINTS, "boxes_per_frame": BOXES, "clouds": "synthetic",
           "device": torch.cuda.get_device_name(dev), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "hbm_gib": round(prop.total_memory / 2 ** 30, 1), "timing": "median of 3 windows >= 0.5 s, sync per iteration"}
    net = standin(cfg).train().to(dev)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    gt, goffs, gcls = boxes_of(cfg, net.anchors.cpu().numpy(), seed=11)
    d = lambda a: torch.from_numpy(a).to(dev)
    step_args = (d(pts), d(offs), d(gt), d(goffs), d(gcls))
    # (a) the stand-in's own iteration
    ex = example_of(net, clouds, dev, metadata=False)
    begin = models.anchor_class_ranges(cfg, [1, 100, 100])
    labels, reg, imp = ops.assign_targets_per_class(net.anchors.to(dev), step_args[2], step_args[3], step_args[4], begin, cfg["group_class_ids"],
                                                    cfg["matched_thresholds"], cfg["unmatched_thresholds"])
    ex.update(labels=labels, reg_targets=reg, importance=imp)
    res["pillars"] = int(ex["voxels"].shape[0])
    res["positives"] = int((labels > 0).sum())
    opt = torch.optim.AdamW([q for q in net.parameters() if q.requires_grad], lr=1e-4, weight_decay=0.01, betas=(0.9, 0.99))
    last = {}

    def standin_step():
        opt.zero_grad(set_to_none=True)
        out = net(ex)
        out["loss"].backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 10.0)
        opt.step()
        last["loss"] = out["loss"].detach()
    torch.cuda.reset_peak_memory_stats()
    r = runs_of(standin_step)
    res["standin_module_graph_fp32"] = dict(r, loss=round(float(last["loss"]), 4), peak_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    del net, opt, ex
    torch.cuda.empty_cache()
    # (b), (c) the device trainer
    for label, dtype in (("fp32", None), ("bf16", torch.bfloat16)):
        det = SecondDetector(cfg)
        det.load_state_dict({k: v for k, v in state.items() if k in det.state_dict()}, strict=False)
        tr = MultiHeadDeviceTrainer(det.to(dev), lr=1e-4, amp_dtype=dtype)
        torch.cuda.reset_peak_memory_stats()
        r = runs_of(lambda: tr.step(*step_args))
        graphed = tr._graphed_rpn is not None and tr._graphed_rpn[1] is not None
        res["device_trainer_" + label] = dict(r, loss=round(tr.loss_dict()["loss"], 4), dense_segment_graphed=graphed,
                                              peak_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
        if dtype is not None:
            res["conv64_layers_alone_" + label] = conv64_alone(det, dtype, res["device_trainer_" + label]["ms_per_iteration"])
        del tr, det
        torch.cuda.empty_cache()
    base = res["standin_module_graph_fp32"]["ms_per_iteration"]
    res["speedup"] = {k: round(base / res["device_trainer_" + k]["ms_per_iteration"], 2) for k in ("fp32", "bf16")}
    res["pfn_layer_alone"] = pfn_alone(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
