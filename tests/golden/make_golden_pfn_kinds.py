"""Produces tests/golden/pfn_kinds.npz by EXECUTING the reference on CPU.  Build container only (needs the reference checkout):

    python tests/golden/make_golden_pfn_kinds.py <path to the reference checkout>      (or SECOND_REFERENCE)

The four pillar encoders of second/pytorch/models/pointpillars.py -- PillarFeatureNet, PillarFeatureNetRadius, PillarFeatureNetOld,
PillarFeatureNetRadiusHeight -- each with ``with_distance`` False and True, on the 40 pillars of up to 12 points of
``make_golden_mhead.pfn_inputs(40, 12, 23)``, 16 channels, seeded weights (one [16, 10] matrix; a variant whose row has K entries
takes its first K columns).  Per variant ``<name>.<d>`` (d = 0 / 1): eval mode in float32 and float64 (seeded running statistics),
train() mode in float64 (``out``, the three gradients of sum(out * w), the running statistics after the call), and the error of the
reference's own float32 run per quantity, as make_golden_pfn_train.py records it.  PillarFeatureNetOld writes the centre offsets
into its input: the x, y columns it leaves behind are recorded too (``<name>.<d>.mutated_xy``), every call gets a fresh copy of the
inputs, and the inputs are stored once, unmodified."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden_mhead import RANGE, VOXEL, pfn_inputs  # noqa: E402
from make_golden_mhead_train import QUANTITIES  # noqa: E402

CHANNELS = 16
NAMES = ("PillarFeatureNet", "PillarFeatureNetRadius", "PillarFeatureNetOld", "PillarFeatureNetRadiusHeight")


def build(cls, dist, dtype, weights, train):
    vfe = cls(num_input_features=4, use_norm=True, num_filters=(CHANNELS,), with_distance=dist, voxel_size=VOXEL, pc_range=RANGE)
    vfe.train(train)
    layer = vfe.pfn_layers[0]
    k = layer.linear.weight.shape[1]
    with torch.no_grad():
        layer.linear.weight.copy_(weights["linear_weight"][:, :k])
        layer.norm.weight.copy_(weights["norm_weight"])
        layer.norm.bias.copy_(weights["norm_bias"])
        layer.norm.running_mean.copy_(weights["running_mean"])
        layer.norm.running_var.copy_(weights["running_var"])
    return vfe.to(dtype), layer, k


def run(cls, dist, dtype, weights, inputs, w, train):
    vfe, layer, k = build(cls, dist, dtype, weights, train)
    v = torch.from_numpy(inputs[0].copy()).to(dtype)
    out = vfe(v, torch.from_numpy(inputs[1]), torch.from_numpy(inputs[2]))
    assert tuple(out.shape) == (inputs[0].shape[0], CHANNELS)
    res = dict(out=out.detach(), k=k, mutated_xy=v[..., :2].detach())
    if train:
        (out * w.to(dtype)).sum().backward()
        res.update(d_linear_weight=layer.linear.weight.grad, d_norm_weight=layer.norm.weight.grad, d_norm_bias=layer.norm.bias.grad,
                   running_mean=layer.norm.running_mean, running_var=layer.norm.running_var, eps=layer.norm.eps,
                   momentum=layer.norm.momentum)
    return res


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["SECOND_REFERENCE"]
    sys.path[:0] = [os.path.join(ROOT, "second.pytorch_amd"), ROOT]
    from second_amd import compat
    compat.install(ref)
    from second.pytorch.models import pointpillars
    gen = torch.Generator().manual_seed(41)
    weights = dict(linear_weight=torch.empty(CHANNELS, 10).uniform_(-0.35, 0.35, generator=gen),
                   norm_weight=torch.empty(CHANNELS).uniform_(0.5, 1.5, generator=gen),
                   norm_bias=torch.empty(CHANNELS).uniform_(-0.3, 0.3, generator=gen),
                   running_mean=torch.empty(CHANNELS).uniform_(-0.5, 0.5, generator=gen),
                   running_var=torch.empty(CHANNELS).uniform_(0.5, 2.0, generator=gen))
    inputs = pfn_inputs(40, 12, 23)
    w = torch.randn(40, CHANNELS, generator=gen)
    out = dict(voxels=inputs[0], num_points=inputs[1], coords=inputs[2], w=w.numpy(), voxel_size=np.array(VOXEL, np.float64),
               pc_range=np.array(RANGE, np.float64))
    for k, t in weights.items():
        out[k] = t.numpy()
    for name in NAMES:
        cls = getattr(pointpillars, name)
        for dist in (False, True):
            key = f"{name}.{int(dist)}."
            e64, e32 = (run(cls, dist, dt, weights, inputs, w, False) for dt in (torch.float64, torch.float32))
            t64, t32 = (run(cls, dist, dt, weights, inputs, w, True) for dt in (torch.float64, torch.float32))
            out[key + "k"] = np.int64(t64["k"])
            out[key + "eval64"] = e64["out"].numpy()
            out[key + "eval32"] = e32["out"].numpy()
            out[key + "f32_err.eval"] = np.float64(np.abs(e64["out"].numpy() - e32["out"].double().numpy()).max() / np.abs(e64["out"].numpy()).max())
            for q in QUANTITIES:
                a, b = t64[q].double().numpy(), t32[q].double().numpy()
                out[key + q] = a
                out[key + "f32_err." + q] = np.float64(np.abs(a - b).max() / np.abs(a).max())
            out["eps"], out["momentum"] = np.float64(t64["eps"]), np.float64(t64["momentum"])
            mutated = not np.array_equal(t32["mutated_xy"].numpy(), inputs[0][..., :2])
            assert mutated == (name == "PillarFeatureNetOld"), (name, mutated)
            if mutated:
                out[key + "mutated_xy"] = t32["mutated_xy"].numpy()
    path = os.path.join(HERE, "pfn_kinds.npz")
    np.savez_compressed(path, **out)
    print({k: (getattr(v, "shape", None) or float(v)) for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
