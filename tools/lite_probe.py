"""Probe: batch-8 car.lite (SimpleVoxelRadius + SpMiddleFHDLite, 160 x 132 map) through
  (a) the module graph of the reference-shaped network object (tests/reference_standin_lite.py): eager, dynamic shapes, ``.dense()``,
      torch RPN and predict -- the only way the network ran before the fused path took it, so this is the baseline;
  (b) ``SecondDetector.forward_points`` replayed from hipGraphs by the bench's in-flight runner (voxelisation included),
in bf16 and fp32 (fp32 storage, split-operand products), medians of three runs of >= 0.5 s after warm-up, plus the per-launch table
of one static forward.  Clouds are synthetic (second_amd.synthetic, cropped to the lite range).
    python tools/lite_probe.py [--out profiles/lite_probe.json]            (prints one JSON line)"""
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
import bench  # noqa: E402
from second_amd import ops, synthetic as syn  # noqa: E402
from second_amd.models import CAR_LITE, InFlightRunner, SecondDetector  # noqa: E402

BATCH, POINTS, VOXELS = 8, 11000, 10000


def runs_of(step, sync, seconds=0.5, runs=3, warmup=10):
    """frames/s: medians of ``runs`` runs of >= ``seconds`` each"""
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
        out.append(n * BATCH / (time.perf_counter() - t0))
    return {"frames_per_s": round(statistics.median(out), 1), "runs": [round(v, 1) for v in out]}


def launch_table(det, points, offsets, reps=20):
    """every traced op of ONE static forward, re-issued ``reps`` times between two events"""
    calls = []

    def note(name, fn, a, kw, res):
        kernel = ""
        if name == "indice_conv":         # (features, weight, nbr_out, num_out, ...): the kernel family the dispatcher picks for the layer
            w, packed = a[1], kw.get("packed")
            plan = ops.indice_conv_plan(w.shape[-2], w.shape[-1], w.numel() // (w.shape[-2] * w.shape[-1]), a[3], w.dtype,
                                        kw.get("out_dtype") or w.dtype, packed is not None)
            kernel = f"{bench.PLAN_NAMES.get(plan, plan)} {w.shape[-2]}->{w.shape[-1]} rows {a[3]}"
        calls.append((name, fn, a, kw, kernel))
    ops.set_op_hook(note)
    try:
        with torch.no_grad():
            det.forward_points(points, offsets, static=True)
        torch.cuda.synchronize()
    finally:
        ops.set_op_hook(None)
    prev = ops.set_rulebook_numbering(det.rulebook_numbering)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = []
    try:
        with torch.no_grad(), ops.fp32_mode("exact" if getattr(det, "fp32_exact", False) else None):
            for name, fn, a, kw, kernel in calls:
                for _ in range(2):
                    fn(*a, **kw)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    fn(*a, **kw)
                e1.record()
                torch.cuda.synchronize()
                ent = {"op": name, "us": round(e0.elapsed_time(e1) * 1e3 / reps, 2)}
                if kernel:
                    ent["kernel"] = kernel
                rows.append(ent)
    finally:
        ops.set_rulebook_numbering(prev)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--inflight", type=int, default=4)
    args = ap.parse_args()
    from lite_helpers import clouds_for, trained_like
    from reference_standin import example_of
    from reference_standin_lite import build_voxelnet_lite
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    clouds = clouds_for(CAR_LITE, range(BATCH), num_points=POINTS, num_voxels=VOXELS)
    like = trained_like(CAR_LITE, clouds[0])
    pts, offs = syn.batch_clouds(clouds)
    points, offsets = torch.from_numpy(pts).to(dev), torch.from_numpy(offs).to(dev)
    prop = torch.cuda.get_device_properties(dev)
    res = {"network": "car.lite", "batch": BATCH, "points_per_cloud": POINTS, "voxels_per_cloud": VOXELS, "clouds": "synthetic",
           "device": torch.cuda.get_device_name(dev), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "hbm_gib": round(prop.total_memory / 2 ** 30, 1), "inflight": args.inflight, "module_graph": {}, "fused_graph": {}, "launches": {}}
    for label, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        # (a) the module graph
        net = build_voxelnet_lite(CAR_LITE)
        net.load_state_dict(like.state_dict())
        net = net.eval().to(dev)
        if dtype != torch.float32:
            net = net.to(dtype)
            for m in net.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.float()
        ex = example_of(net, clouds, dev, dtype=dtype)
        try:
            with torch.no_grad():
                n_ref = sum(int(r["scores"].shape[0]) for r in net(ex))
                res["module_graph"][label] = dict(runs_of(lambda: net(ex), torch.cuda.synchronize, warmup=3), detections=n_ref)
        except Exception as e:   # noqa: BLE001 -- a module graph torch cannot run in this dtype is recorded, not hidden
            res["module_graph"][label] = {"error": f"{type(e).__name__}: {e}"[:300]}
        del net
        # (b) forward_points from hipGraphs, steps in flight
        det = SecondDetector(CAR_LITE)
        det.load_state_dict(like.state_dict())
        det = det.eval().to(dev).prepare_inference(dtype)
        with torch.no_grad():
            det.calibrate(points, offsets)
            runner = InFlightRunner(det, points, offsets, inflight=args.inflight, serialize_rpn=True)
            r = runs_of(runner.step, torch.cuda.synchronize)
            runner.synchronize()
            outs = runner.outputs[-1]
            r["detections"] = int(outs["valid"].sum().item())
            r["arithmetic"] = det.arithmetic()
            res["fused_graph"][label] = r
            res["launches"][label] = launch_table(det, points, offsets)
        del runner, det
        torch.cuda.empty_cache()
    res["speedup"] = {}
    for label in res["fused_graph"]:
        base = res["module_graph"].get(label, {}).get("frames_per_s") or res["module_graph"]["fp32"].get("frames_per_s")
        if base:
            res["speedup"][label] = round(res["fused_graph"][label]["frames_per_s"] / base, 2)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ok = all(v > 1.0 for v in res["speedup"].values()) and len(res["speedup"]) == 2
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
