"""Produces tests/golden/mhead.npz by EXECUTING the reference on CPU.  Build container only (needs the reference checkout):

    python tests/golden/make_golden_mhead.py [path to the reference checkout]

  * ``PillarFeatureNetRadius.forward`` (second/pytorch/models/pointpillars.py:240-325) in eval mode on 64 pillars of up to 60
    points of the nuscenes/all.pp.mhead grid (0.25 m pillars, +-50 m): every point lies inside its pillar and inside the range, the
    point counts cover 1 and 60, one pillar touches the sensor axis (radii down to a few centimetres; a point AT x = y = 0 is the GPU
    test's own case); seeded weights and running statistics;
  * the anchors of ``all.pp.mhead.config``'s target assigner (second/core/target_assigner.py:169-207) at a reduced geometry: range
    +-10 m, the small classes' +-8 m, maps [1, 20, 20] / [1, 32, 32]: 4 800 + 8 192 anchors.

No network weights besides the PFN layer's (64 x 8 + 4 x 64 values)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

RANGE, VOXEL = (-50.0, -50.0, -5.0, 50.0, 50.0, 3.0), (0.25, 0.25, 8.0)


def pfn_inputs(p=64, t=60, seed=21):
    g = np.random.default_rng(seed)
    num = g.integers(1, t + 1, p).astype(np.int32)
    num[:4], num[4:8] = 1, t
    cx, cy = g.integers(0, 400, p), g.integers(0, 400, p)
    cx[8], cy[8] = 200, 200                                # the pillar whose corner is the sensor: radii down to ~0
    coords = np.stack([g.integers(0, 2, p), np.zeros(p, np.int64), cy, cx], 1).astype(np.int32)     # (b, z, y, x)
    v = np.zeros((p, t, 4), np.float32)
    v[..., 0] = RANGE[0] + (cx[:, None] + g.uniform(0.02, 0.98, (p, t))) * VOXEL[0]
    v[..., 1] = RANGE[1] + (cy[:, None] + g.uniform(0.02, 0.98, (p, t))) * VOXEL[1]
    v[..., 2] = g.uniform(RANGE[2], RANGE[5], (p, t))
    v[..., 3] = g.uniform(0, 1, (p, t))
    v *= (np.arange(t)[None, :] < num[:, None])[..., None]
    return v.astype(np.float32), num, coords


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SECOND_REFERENCE", "/root/reference")
    sys.path[:0] = [os.path.join(ROOT, "second.pytorch_amd"), ROOT]
    from second_amd import compat
    compat.install(ref)
    from google.protobuf import text_format
    from second.protos import pipeline_pb2
    from second.builder import target_assigner_builder
    from second.pytorch.builder import box_coder_builder
    from second.pytorch.models.pointpillars import PillarFeatureNetRadius
    out = {}
    # ---- PillarFeatureNetRadius
    torch.manual_seed(5)
    vfe = PillarFeatureNetRadius(num_input_features=4, use_norm=True, num_filters=(64,), with_distance=False, voxel_size=VOXEL,
                                 pc_range=RANGE).eval()
    gen = torch.Generator().manual_seed(6)
    norm = vfe.pfn_layers[0].norm
    with torch.no_grad():
        norm.weight.copy_(torch.empty(64).uniform_(0.5, 1.5, generator=gen))
        norm.bias.copy_(torch.empty(64).uniform_(-0.3, 0.3, generator=gen))
        norm.running_mean.copy_(torch.empty(64).uniform_(-0.5, 0.5, generator=gen))
        norm.running_var.copy_(torch.empty(64).uniform_(0.5, 1.5, generator=gen))
    v, num, coords = pfn_inputs()
    with torch.no_grad():
        r = vfe(torch.from_numpy(v), torch.from_numpy(num), torch.from_numpy(coords))
    assert tuple(r.shape) == (64, 64)
    out.update(pfn_voxels=v, pfn_num_points=num, pfn_coords=coords, pfn_out=r.numpy().astype(np.float32),
               pfn_eps=np.float32(norm.eps))
    for k, t in vfe.state_dict().items():
        if t.is_floating_point():
            out["pfn_sd." + k] = t.numpy().astype(np.float32)
    # ---- anchors of the config's target assigner at a reduced geometry
    cfg = pipeline_pb2.TrainEvalPipelineConfig()
    text_format.Merge(open(os.path.join(ref, "second/configs/nuscenes/all.pp.mhead.config")).read(), cfg)
    model_cfg = cfg.model.second
    for cs in model_cfg.target_assigner.class_settings:
        ar = cs.anchor_generator_range.anchor_ranges
        small = abs(ar[0]) == 40
        lim = 8.0 if small else 10.0
        ar[0], ar[1], ar[3], ar[4] = -lim, -lim, lim, lim
        cs.feature_map_size[:] = [1, 32, 32] if small else [1, 20, 20]
    ta = target_assigner_builder.build(model_cfg.target_assigner, np.array([-10, -10, 10, 10], np.float32),
                                       box_coder_builder.build(model_cfg.box_coder))
    anchors = ta.generate_anchors([1, 20, 20])["anchors"].reshape(-1, 7)
    assert anchors.shape == (4800 + 8192, 7), anchors.shape
    out["anchors_small_geometry"] = anchors.astype(np.float32)
    out["anchor_classes"] = np.array(list(ta.classes))
    path = os.path.join(HERE, "mhead.npz")
    np.savez_compressed(path, **out)
    print({k: getattr(v, "shape", v) for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
