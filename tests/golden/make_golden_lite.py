"""Produces tests/golden/simple_voxel_radius.npz by EXECUTING the reference's ``SimpleVoxelRadius.forward``
(second/pytorch/models/voxel_encoder.py:228-255) on CPU.  Build container only (needs the reference checkout):

    python tests/golden/make_golden_lite.py [path to the reference checkout]

Inputs: voxel tensors with 1 and 5 point slots, ragged point counts (padded slots zero, as the voxeliser leaves them), rows whose
points have x = y = 0 (radius exactly 0) and rows with large |x| (the squares stay finite in fp32)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def inputs(t, n, seed):
    g = np.random.default_rng(seed)
    num = g.integers(1, t + 1, n).astype(np.int32)
    v = np.zeros((n, t, 4), np.float32)
    v[..., 0] = g.uniform(0, 70.4, (n, t))
    v[..., 1] = g.uniform(-40, 40, (n, t))
    v[..., 2] = g.uniform(-3, 1, (n, t))
    v[..., 3] = g.uniform(0, 1, (n, t))
    v[:16, :, :2] = 0.0                                   # on the sensor axis: r = 0
    v[16:32, :, 0] = g.uniform(1e4, 1e6, (16, t))         # far outside any range: large |x|
    v[32:48, :, 0] *= -1.0
    v[48:56, :, 1] = 0.0                                  # r = |x|
    v *= (np.arange(t)[None, :] < num[:, None])[..., None]
    return v.astype(np.float32), num


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SECOND_REFERENCE", "/root/reference")
    sys.path[:0] = [os.path.join(ROOT, "second.pytorch_amd"), ROOT]
    from second_amd import compat
    compat.install(ref)
    from second.pytorch.models.voxel_encoder import SimpleVoxelRadius
    vfe = SimpleVoxelRadius(num_input_features=4)
    out = {}
    for t, n, seed in ((1, 300, 11), (5, 400, 12)):
        v, num = inputs(t, n, seed)
        with torch.no_grad():
            r = vfe(torch.from_numpy(v), torch.from_numpy(num), None)
        out[f"voxels_t{t}"], out[f"num_points_t{t}"], out[f"out_t{t}"] = v, num, r.numpy().astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "simple_voxel_radius.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
