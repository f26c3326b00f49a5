"""Probe: batch-8 nuscenes/all.pp.mhead (PillarFeatureNetRadius + PointPillarsScatter + RPNNoHead + two heads, 324 800 anchors) through
  (a) the module graph of the reference-shaped network object (tests/reference_standin_mhead.py): eager, torch formulations, torch
      predict on the concatenated heads -- the only way the network ran before the fused path took it, so this is the baseline;
  (b) ``SecondDetector.forward_points`` replayed from hipGraphs with four steps in flight (voxelisation included),
in fp32 and bf16, medians of three windows of >= 0.5 s after warm-up; and
  (c) the one-segment form of the multi-tensor select (sec_predict_select_segments) timed against sec_predict_select at largea's
      head shape (12 x 100 x 100 anchors, 10 classes, batch 8, bf16): same algorithm, addresses through the segment table.
Clouds are synthetic (second_amd.synthetic).
    python tools/mhead_probe.py [--out profiles/mhead_probe_bs8.json]            (prints one JSON line)"""
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
from second_amd import ops, synthetic as syn  # noqa: E402
from second_amd.models import ALL_PP_MHEAD, InFlightRunner, SecondDetector  # noqa: E402

BATCH, POINTS = 8, 60000


def runs_of(step, sync, seconds=0.5, runs=3, warmup=10, per_step=BATCH):
    """units/s (frames by default): medians of ``runs`` windows of >= ``seconds`` each"""
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
    return {"per_s": round(statistics.median(out), 1), "runs": [round(v, 1) for v in out]}


def select_one_segment(dev, calls=50):
    """sec_predict_select vs sec_predict_select_segments (S = 1) on the same views.  Device time per call: ``calls`` back-to-back calls
    captured into one hipGraph each, replays timed between two events (the Python wrappers' host time is not in it)."""
    b, a, h, w, nc = BATCH, 12, 100, 100, 10
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.randn(b, 256, h, w, device=dev, generator=g)
    t[:, a * 7:a * (7 + nc)] = t[:, a * 7:a * (7 + nc)] * 0.8 - 6.0                # a trained-like head: a few hundred candidates per frame
    t = t.bfloat16().contiguous(memory_format=torch.channels_last)
    cls = t[:, a * 7:a * (7 + nc)].reshape(b, a, nc, h, w).permute(0, 1, 3, 4, 2)
    one = ops.predict_select(cls, 1000, 0.05)
    seg = ops.predict_select([cls], 1000, 0.05)
    same = all(torch.equal(x, y) for x, y in zip(one, seg))

    def graph_of(arg):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.predict_select(arg, 1000, 0.05)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with ops.rt.capture_guard(), torch.cuda.graph(gr, capture_error_mode="thread_local"):
            keep = [ops.predict_select(arg, 1000, 0.05) for _ in range(calls)]
        return gr, keep

    def us_per_call(gr):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for _ in range(3):                            # three windows of >= 0.5 s
            n, t0 = 0, time.perf_counter()
            e0.record()
            while True:
                gr.replay()
                n += 1
                if n % 16 == 0:
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= 0.5:
                        break
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / (n * calls))
        return round(statistics.median(out), 2), [round(v, 2) for v in out]
    g_old, k_old = graph_of(cls)
    g_new, k_new = graph_of([cls])
    for _ in range(5):
        g_old.replay(), g_new.replay()
    torch.cuda.synchronize()
    old, old_runs = us_per_call(g_old)
    new, new_runs = us_per_call(g_new)
    return {"shape": [b, a, h, w, nc], "dtype": "bf16", "candidates_per_frame": [int(v) for v in one[3].tolist()], "bit_equal": same,
            "single_map_us_per_call": old, "single_map_runs": old_runs, "one_segment_us_per_call": new, "one_segment_runs": new_runs,
            "one_segment_over_single_map_time": round(new / old, 3), "timing": f"{calls} calls per hipGraph, replays between two events"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--inflight", type=int, default=4)
    args = ap.parse_args()
    from mhead_helpers import trained_like_standin
    from reference_standin import example_of
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    clouds = [syn.syn_nusc_cloud(s, num_points=POINTS, point_cloud_range=tuple(ALL_PP_MHEAD["point_cloud_range"])) for s in range(BATCH)]
    pts, offs = syn.batch_clouds(clouds)
    points, offsets = torch.from_numpy(pts).to(dev), torch.from_numpy(offs).to(dev)
    prop = torch.cuda.get_device_properties(dev)
    res = {"network": "nuscenes/all.pp.mhead", "batch": BATCH, "points_per_cloud": POINTS, "clouds": "synthetic",
           "device": torch.cuda.get_device_name(dev), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "hbm_gib": round(prop.total_memory / 2 ** 30, 1), "inflight": args.inflight, "module_graph": {}, "fused_graph": {}}
    like = trained_like_standin(ALL_PP_MHEAD, clouds[0])
    state = {k: v.clone() for k, v in like.state_dict().items()}
    for label, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        # (a) the module graph
        net = like if dtype == torch.float32 else None
        if net is not None:
            ex = example_of(net, clouds, dev, dtype=dtype)
            with torch.no_grad():
                n_ref = sum(int(r["scores"].shape[0]) for r in net(ex))
                r = runs_of(lambda: net(ex), torch.cuda.synchronize, warmup=3)
            res["module_graph"][label] = {"frames_per_s": r["per_s"], "runs": r["runs"], "detections": n_ref}
        # (b) forward_points from hipGraphs, steps in flight
        det = SecondDetector(ALL_PP_MHEAD)
        det.load_state_dict({k: v for k, v in state.items() if k in det.state_dict()}, strict=False)
        det = det.eval().to(dev).prepare_inference(dtype)
        with torch.no_grad():
            runner = InFlightRunner(det, points, offsets, inflight=args.inflight)
            r = runs_of(runner.step, torch.cuda.synchronize)
            runner.synchronize()
            outs = runner.outputs[-1]
            res["fused_graph"][label] = {"frames_per_s": r["per_s"], "runs": r["runs"], "detections": int(outs["valid"].sum().item()),
                                         "arithmetic": det.arithmetic()}
        del runner, det
        torch.cuda.empty_cache()
    base = res["module_graph"]["fp32"]["frames_per_s"]       # (the module graph is an fp32 object: one baseline for both)
    res["speedup"] = {label: round(v["frames_per_s"] / base, 2) for label, v in res["fused_graph"].items()}
    res["select_one_segment"] = select_one_segment(dev)
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
