"""Probe: the PillarFeatureNet family (plain, radius, old, radius_height; each also with_distance) at nuScenes size.
  (a) the layer alone at 4 x 30 000 pillars x 60 slots, 64 channels: forward (eval) and forward + backward (train) of every kind on the
      kernels (sec_pfn_kind_*) against the module's torch formulation (the reference's
      materialised [P, T, C] tensor), with the peak memory of each above the resident inputs;
  (b) ``SecondDetector.forward_points`` at models.ALL_PP_MIDA (PillarFeatureNetOld, 400 x 400 pillars, 200 000 anchors), batch 8, bf16.
Medians of three windows of >= 0.5 s after warm-up.  No figure here is a pass criterion.
    python tools/pfn_kinds_probe.py [--out profiles/pfn_kinds_probe.json] [--kinds plain,radius]       (prints one JSON line)"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "second.pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from second_amd import models, synthetic as syn  # noqa: E402

FRAMES, PILLARS, SLOTS, CHANNELS = 4, 30000, 60, 64
CLASSES = {"plain": "PillarFeatureNet", "radius": "PillarFeatureNetRadius", "old": "PillarFeatureNetOld",
           "radius_height": "PillarFeatureNetRadiusHeight"}


def ms_of(step, seconds=0.5, runs=3, warmup=3):
    """ms per call: median of ``runs`` windows of >= ``seconds`` each, one device sync per window of queued calls"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(4):
                step()
            n += 4
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
        out.append(1e3 * (time.perf_counter() - t0) / n)
    return round(statistics.median(out), 3), [round(v, 3) for v in out]


def peak_of(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def pillars(seed=0):
    """[FRAMES * PILLARS, SLOTS, 4] pillars on the 0.25 m grid of +-50 m: 1 .. SLOTS points, points inside their pillar."""
    g = torch.Generator().manual_seed(seed)
    p = FRAMES * PILLARS
    n = torch.randint(1, SLOTS + 1, (p,), generator=g)
    cell = torch.stack([torch.randperm(160000, generator=g)[:PILLARS] for _ in range(FRAMES)]).reshape(-1)
    coords = torch.stack([torch.arange(FRAMES).repeat_interleave(PILLARS), torch.zeros(p, dtype=torch.long), cell // 400, cell % 400], 1).int()
    v = torch.rand(p, SLOTS, 4, generator=g)
    v[..., 0] = -50 + (coords[:, 3:4] + v[..., 0]) * 0.25
    v[..., 1] = -50 + (coords[:, 2:3] + v[..., 1]) * 0.25
    v[..., 2] = v[..., 2] * 8 - 5
    v *= (torch.arange(SLOTS).view(1, -1) < n.view(-1, 1)).unsqueeze(-1)
    return v.cuda(), n.int().cuda(), coords.cuda()


def layer_rows(kinds, distance=(False, True)):
    v, n, co = pillars()
    w = torch.randn(v.shape[0], CHANNELS, generator=torch.Generator().manual_seed(1)).cuda()
    rows = {}
    for name in kinds:
        for dist in distance:
            row = {}
            for backend in ("hip", "torch"):
                torch.manual_seed(0)
                m = models.VFES[CLASSES[name]](4, [CHANNELS], (0.25, 0.25, 8), (-50, -50, -5, 50, 50, 3), **({"with_distance": True} if dist else {}))
                m = m.cuda()
                m.train_backend = backend

                def fwd():
                    # eval mode: the kernels serve calls without autograd, the torch formulation calls with it (nothing requires a
                    # gradient here, so no graph is kept)
                    with torch.set_grad_enabled(backend == "torch"):
                        return m(v, n, co)

                def fwd_bwd():
                    for p in m.parameters():
                        p.grad = None
                    (m(v, n, co) * w).sum().backward()
                m.eval().requires_grad_(False)
                ms, runs = ms_of(fwd)
                row[backend] = {"forward_ms": ms, "forward_runs_ms": runs, "forward_peak_mib": peak_of(fwd)}
                m.train().requires_grad_(True)
                ms, runs = ms_of(fwd_bwd)
                row[backend].update({"forward_backward_ms": ms, "forward_backward_runs_ms": runs, "forward_backward_peak_mib": peak_of(fwd_bwd)})
                del m
                torch.cuda.empty_cache()
            rows[name + ("+dist" if dist else "")] = row
            print(name, dist, row, file=sys.stderr, flush=True)
    return rows


def detector_row(batch=8, points=60000):
    cfg = models.ALL_PP_MIDA
    torch.manual_seed(0)
    det = models.SecondDetector(cfg)
    syn.randomise_like_trained(det, seed=1)
    det = det.cuda().eval().prepare_inference(torch.bfloat16)
    clouds = [syn.syn_nusc_cloud(s, num_points=points, point_cloud_range=tuple(cfg["point_cloud_range"])) for s in range(batch)]
    pts, offs = syn.batch_clouds(clouds)
    pts, offs = torch.from_numpy(pts).cuda(), torch.from_numpy(offs).cuda()
    with torch.no_grad():
        replay, _ = det.make_graphed(pts, offs)
        ms, runs = ms_of(replay)
    return {"config": cfg["name"], "batch": batch, "points_per_frame": points, "dtype": "bf16", "mode": "graph", "ms_per_step": ms,
            "runs_ms": runs, "frames_per_s": round(1e3 * batch / ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--kinds", default=",".join(CLASSES))
    ap.add_argument("--no-detector", action="store_true")
    ap.add_argument("--no-distance", action="store_true", help="the rows without the distance entry only")
    args = ap.parse_args()
    res = {"probe": "pfn_kinds", "device": torch.cuda.get_device_name(0), "frames": FRAMES, "pillars_per_frame": PILLARS, "slots": SLOTS,
           "channels": CHANNELS, "layer": layer_rows([k for k in args.kinds.split(",") if k], (False,) if args.no_distance else (False, True))}
    if not args.no_detector:
        res["forward_points"] = detector_row()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
