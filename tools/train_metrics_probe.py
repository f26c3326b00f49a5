#!/usr/bin/env python3
"""Probe: ``VoxelNet.update_metrics`` (voxelnet.py:654-679), the last call of the reference's training iteration, three ways:

  reference   the reference's formulation on GPU tensors -- torchplus.metrics' own classes under the reference's own method where a
              reference checkout is present (SECOND_REFERENCE), else the torch formulation of tests/train_metrics_helpers.py that
              tests/test_train_metrics_host.py holds to the recorded reference exactly (same operations, same 23 host reads);
  update      second_amd.train_metrics.DeviceTrainMetrics.update: two launches, one copy into pinned memory, one event wait;
  accumulate  the two launches alone, replayed from a hipGraph (no read).

Geometries: car.fhd (B 4, N 70 400, C 1) and nuScenes all.fhd (B 4, N 307 520, C 10); random N(0, 2) logits, labels with about
0.1 % positives and 10 % ignored.  Seconds per call, medians of three windows of >= 0.5 s after a warm-up.  The host-read counts
are taken from the code, not from a trace.  ``--loop``: the fused car.fhd training iteration (net(example), backward, clip,
AdamW, update_metrics; stand-in network, batch 4, synthetic example) with and without the hook.  What could not be taken reads
"not measured".

    python tools/train_metrics_probe.py [--out profiles/train_metrics_probe.json] [--loop]   (one JSON line)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "second.pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NOT_MEASURED = "not measured"
GEOMETRIES = {"car.fhd": (4, 70400, 1), "nusc_all.fhd": (4, 307520, 10)}


def per_call(fn, window=0.5):
    """Seconds per call: median of three windows of >= ``window`` s, each closed by a device synchronisation."""
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(10):
                fn()
            n += 10
            if time.perf_counter() - t0 >= window:
                break
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / n)
    return statistics.median(runs), runs


def reference_holder(num_class, H):
    """-> (holder, which): real torchplus.metrics modules under the reference's unbound method when a checkout is present."""
    ref = os.environ.get("SECOND_REFERENCE", "")
    if ref and os.path.isdir(os.path.join(ref, "second")):
        try:
            import types
            from second_amd import compat
            compat.install(ref)
            from second.pytorch.models.voxelnet import VoxelNet
            from torchplus import metrics
            h = H.holder(num_class, None, {
                "rpn_acc": metrics.Accuracy(dim=-1, encode_background_as_zeros=True),
                "rpn_metrics": metrics.PrecisionRecall(dim=-1, thresholds=list(H.DEFAULT_THRESHOLDS), use_sigmoid_score=True,
                                                       encode_background_as_zeros=True),
                "rpn_cls_loss": metrics.Scalar(), "rpn_loc_loss": metrics.Scalar()})
            h.update_metrics = types.MethodType(VoxelNet.update_metrics, h)
            return h, "the reference's own classes and method"
        except Exception as e:                                      # noqa: BLE001 -- a probe: say why and measure the stand-in
            print("reference checkout not usable:", repr(e), file=sys.stderr)
    return H.holder(num_class), "torch formulation of tests/train_metrics_helpers.py (pinned to the recorded reference on the CPU)"


def geometry(name, b, n, c):
    import numpy as np
    import torch
    import train_metrics_helpers as H
    from second_amd import runtime as rt
    from second_amd.train_metrics import DeviceTrainMetrics
    rng = np.random.default_rng(7)
    logits = torch.from_numpy(rng.normal(0, 2, (b, n, c)).astype(np.float32)).cuda()
    u = rng.uniform(size=(b, n))
    lab = np.zeros((b, n), np.int32)
    lab[u < 0.10] = -1
    lab[u > 0.999] = rng.integers(1, c + 1, int((u > 0.999).sum()))
    labels = torch.from_numpy(lab).cuda()
    cared = labels >= 0
    cls_loss, loc_loss = torch.tensor(0.7).cuda(), torch.tensor(1.3).cuda()
    args = (cls_loss, loc_loss, logits, labels, cared)
    res = {"batch": b, "anchors_per_frame": n, "num_class": c, "working_set_mb": round((logits.numel() * 4 + labels.numel() * 5) / 1e6, 1),
           "positives_share": round(float((lab > 0).mean()), 5)}
    holder, which = reference_holder(c, H)
    holder = holder.cuda()
    med, runs = per_call(lambda: holder.update_metrics(*args))
    res["reference"] = {"what": which, "seconds_per_call": med, "windows": runs, "host_reads_per_call": H.HOST_READS_REFERENCE}
    m = DeviceTrainMetrics()
    med, runs = per_call(lambda: m.update(*args))
    res["update"] = {"seconds_per_call": med, "windows": runs, "host_reads_per_call": H.HOST_READS_DEVICE, "launches_per_call": 2}
    # same values after the same number of calls is not the point here (the tests hold that); agreement on one fresh update is cheap to show
    a, bnet = DeviceTrainMetrics(), H.holder(c).cuda()
    res["one_update_equal"] = json.dumps(a.update(*args), sort_keys=True) == json.dumps(bnet.update_metrics(*args), sort_keys=True)
    m.accumulate(*args)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with rt.capture_guard(), torch.cuda.graph(graph):
        m.accumulate(*args)
    med, runs = per_call(graph.replay)
    res["accumulate_graph_replay"] = {"seconds_per_call": med, "windows": runs, "host_reads_per_call": 0}
    res["speedup_update_vs_reference"] = round(res["reference"]["seconds_per_call"] / res["update"]["seconds_per_call"], 2)
    return res


def loop_figure(steps_window=0.5):
    """Samples/s of the fused car.fhd iteration with the network's own update_metrics and with the hook (batch 4)."""
    import torch
    import train_metrics_helpers as H
    from reference_standin import build_voxelnet, train_example_of
    from second_amd import compat, synthetic as syn
    from second_amd.models import CAR_FHD
    out = {}
    for label, hook in (("without_hook", False), ("with_hook", True)):
        torch.manual_seed(0)
        net = H.attach_metrics(build_voxelnet(CAR_FHD)).cuda().train()
        seeds = (0, 1, 2, 3)
        ex = train_example_of(net, [syn.syn_kitti_cloud(s) for s in seeds], [syn.syn_kitti_boxes(s, 10) for s in seeds], torch.device("cuda"))
        compat.accelerate_model(net, train_dtype=torch.bfloat16, train_metrics=hook)
        opt = torch.optim.AdamW(net.parameters(), lr=1e-4)

        def step():
            r = net(ex)
            r["loss"].backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), 10.0)
            opt.step()
            opt.zero_grad()
            return net.update_metrics(r["cls_loss_reduced"], r["loc_loss_reduced"], r["cls_preds"], ex["labels"], r["cared"])
        med, runs = per_call(step, steps_window)
        st = net._second_amd_engine.stats
        out[label] = {"seconds_per_iteration": med, "windows": runs, "samples_per_s": round(len(seeds) / med, 1),
                      "train_calls": st.get("train_calls"), "original_calls": st.get("original_calls"),
                      "train_metrics_calls": st.get("train_metrics_calls"), "train_metrics_fallbacks": st.get("train_metrics_fallbacks"),
                      "train_metrics_fallback_reason": st.get("train_metrics_fallback_reason")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_metrics_probe.json"))
    ap.add_argument("--loop", action="store_true")
    a = ap.parse_args()
    import torch
    res = {"probe": "train_metrics", "sampling": "median of three windows of >= 0.5 s after a warm-up, seconds per call",
           "host_reads_counted_from": "voxelnet.py:654-679 + torchplus/metrics.py (reference), second_amd/train_metrics.py (device)"}
    if not torch.cuda.is_available():
        res.update({k: NOT_MEASURED for k in list(GEOMETRIES) + ["loop_car_fhd_bs4"]})
    else:
        res["device"] = torch.cuda.get_device_name(0)
        for name, (b, n, c) in GEOMETRIES.items():
            res[name] = geometry(name, b, n, c)
        res["loop_car_fhd_bs4"] = NOT_MEASURED
        if a.loop:
            try:
                res["loop_car_fhd_bs4"] = loop_figure()
            except Exception as e:                                  # noqa: BLE001 -- the figure is optional, the reason is part of the record
                res["loop_car_fhd_bs4"] = f"{NOT_MEASURED}: {type(e).__name__}: {e}"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
