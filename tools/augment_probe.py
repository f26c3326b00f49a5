"""Probe: one DeviceAugmenter call at batch 8 on synthetic car.fhd clouds (17 000 points, 40 boxes per frame, 100 tries, the noise
settings of car.fhd.config): eager and replayed from a hipGraph, plus ``draw``; after warm-up, medians of three windows of >= 0.5 s.
    python tools/augment_probe.py [--out profiles/augment_probe_car_fhd_bs8.json]
With ``--reference DIR`` (a checkout of the reference; no GPU needed) it times instead ONE sample of the same batch through the
reference's own noise_per_object_v3_ + random_flip + global_rotation_v2 + global_scaling_v2 + global_translate_ on the CPU, the way
they run in this project's containers: numba's jit stubbed by second_amd.compat, i.e. plain Python -- not a numba figure.  Both
modes merge their keys into ``--out``."""
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
from second_amd import synthetic as syn  # noqa: E402

BATCH, TRIES = 8, 100
CFG = dict(gt_rotation_noise=(-0.78539816, 0.78539816), gt_loc_noise_std=(1.0, 1.0, 0.5), global_rotation_noise=(-0.78539816, 0.78539816),
           global_scaling_noise=(0.95, 1.05), global_translate_noise_std=(0.0, 0.0, 0.0), random_flip_x=False, random_flip_y=True)


def inputs():
    pts, offs = syn.batch_clouds([syn.syn_kitti_cloud(s) for s in range(BATCH)])
    boxes = [syn.syn_kitti_boxes(s) for s in range(BATCH)]
    goffs = np.concatenate([[0], np.cumsum([len(b) for b in boxes])]).astype(np.int32)
    return pts, offs, np.concatenate(boxes).astype(np.float32), goffs


def windows(step, sync, seconds=0.5, runs=3, warmup=20):
    """microseconds per call: medians of ``runs`` windows of >= ``seconds`` each"""
    for _ in range(warmup):
        step()
    sync()
    out = []
    for _ in range(runs):
        n, t0 = 0, time.perf_counter()
        while True:
            step()
            n += 1
            if n % 16 == 0:
                sync()
                if time.perf_counter() - t0 >= seconds:
                    break
        sync()
        out.append((time.perf_counter() - t0) / n * 1e6)
    return {"us_per_call": round(statistics.median(out), 1), "windows": [round(v, 1) for v in out]}


def device_part():
    import torch
    from second_amd import runtime as rt
    from second_amd.augment import DeviceAugmenter
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pts, offs, gt, goffs = (torch.from_numpy(a).to(dev) for a in inputs())
    aug = DeviceAugmenter(point_cloud_range=syn.CAR_FHD_RANGE, num_try=TRIES, **CFG)
    gen = torch.Generator(device=dev).manual_seed(0)
    aug.draw(gen, num_boxes=gt.shape[0], batch_size=BATCH)
    sync = torch.cuda.synchronize
    res = {"batch": BATCH, "points": int(pts.shape[0]), "boxes": int(gt.shape[0]), "tries": TRIES, "clouds": "synthetic",
           "device": torch.cuda.get_device_name(dev)}
    out = aug(pts, offs, gt, goffs)
    res["boxes_kept"] = int(out[3][-1].item())
    res["eager"] = windows(lambda: aug(pts, offs, gt, goffs), sync)
    res["draw"] = windows(lambda: aug.draw(gen), sync)
    graph = torch.cuda.CUDAGraph()
    with rt.capture_guard(), torch.cuda.graph(graph):
        aug(pts, offs, gt, goffs)
    res["graph_replay"] = windows(graph.replay, sync)
    res["graph_replay"]["us_per_sample"] = round(res["graph_replay"]["us_per_call"] / BATCH, 2)
    return res


def reference_part(ref):
    from second_amd import compat
    compat.install(ref)
    from second.core import preprocess as prep
    pts, offs, gt, goffs = inputs()
    p, b = pts[offs[0]:offs[1]].copy(), gt[goffs[0]:goffs[1]].copy()
    np.random.seed(0)
    t0 = time.perf_counter()
    prep.noise_per_object_v3_(b, p, None, rotation_perturb=list(CFG["gt_rotation_noise"]), center_noise_std=list(CFG["gt_loc_noise_std"]),
                              global_random_rot_range=[0.0, 0.0], group_ids=None, num_try=TRIES)
    t1 = time.perf_counter()
    b, p = prep.random_flip(b, p, 0.5, CFG["random_flip_x"], CFG["random_flip_y"])
    b, p = prep.global_rotation_v2(b, p, *CFG["global_rotation_noise"])
    b, p = prep.global_scaling_v2(b, p, *CFG["global_scaling_noise"])
    prep.global_translate_(b, p, list(CFG["global_translate_noise_std"]))
    t2 = time.perf_counter()
    return {"reference_cpu_plain_python": {"what": "one sample (frame 0 of the batch) through the reference's functions with numba's jit stubbed "
                                                   "(second_amd.compat): plain Python on this CPU, one run, not a numba figure",
                                           "points": int(len(p)), "boxes": int(len(b)), "tries": TRIES,
                                           "noise_per_object_v3_s": round(t1 - t0, 3), "global_stages_s": round(t2 - t1, 4)}}


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
