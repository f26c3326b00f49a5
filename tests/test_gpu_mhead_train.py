"""Training nuscenes/all.pp.mhead on the device: sec_pfn_radius_train_fwd / _bwd against the reference layer in float64 (fixture
tests/golden/mhead_train.npz, recorded by make_golden_mhead_train.py) and against the module's own float64 formulation at the shapes
where the kernels take another path, and training.MultiHeadDeviceTrainer at a reduced geometry in fp32 and bf16.

Bounds of the kernel tests, per quantity, as max-abs error over max-abs value: the larger of
  * the tolerance the nine-input kernels are held to (test_gpu_train.py::test_pfn_training_kernels_vs_torch_autograd: out 2e-4,
    gradients 2e-3, running statistics 1e-5) -- the same arithmetic with one product fewer -- and
  * four times the error a float32 run of the reference formulation itself shows against float64 (recorded in the fixture, or
    measured in the test): another summation order is legitimate, a worse order of error is not.
Trainer bounds: loss 1e-4 relative, every gradient 1e-3 of its max-abs value (captured versus eager)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from mhead_train_helpers import GT_CLASSES, RANGE, VOXEL, ragged_pillars, small_batch, small_cfg

pytestmark = pytest.mark.gpu

PROJECT_TOL = {"out": 2e-4, "d_linear_weight": 2e-3, "d_norm_weight": 2e-3, "d_norm_bias": 2e-3, "running_mean": 1e-5, "running_var": 1e-5}


def _rel(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert a.shape == ref.shape
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def _run_layer(device, dtype, backend, weights, vox, num, coors, w, channels):
    """One training forward + backward of models.PillarFeatureNetRadius -> the six quantities and the output's grad_fn name."""
    from second_amd.models import PillarFeatureNetRadius
    net = PillarFeatureNetRadius(4, (channels,), VOXEL, RANGE).train()
    net.train_backend = backend
    layer = net.pfn_layers[0]
    with torch.no_grad():
        layer.linear.weight.copy_(weights["linear_weight"])
        layer.norm.weight.copy_(weights["norm_weight"])
        layer.norm.bias.copy_(weights["norm_bias"])
    net = net.to(device=device, dtype=dtype)
    out = net(vox.to(device=device, dtype=dtype), num.to(device), coors.to(device))
    (out * w.to(device=device, dtype=dtype)).sum().backward()
    assert int(layer.norm.num_batches_tracked) == 1
    res = dict(out=out.detach(), d_linear_weight=layer.linear.weight.grad, d_norm_weight=layer.norm.weight.grad,
               d_norm_bias=layer.norm.bias.grad, running_mean=layer.norm.running_mean, running_var=layer.norm.running_var)
    return {k: v.detach().double().cpu() for k, v in res.items()}, type(out.grad_fn).__name__


def test_radius_training_kernels_match_the_reference_layer_in_float64(golden):
    g = golden("mhead_train")
    assert tuple(g["voxel_size"]) == VOXEL and tuple(g["pc_range"]) == RANGE and float(g["eps"]) == 1e-3 and float(g["momentum"]) == 0.01
    weights = {k: torch.from_numpy(g[k]) for k in ("linear_weight", "norm_weight", "norm_bias")}
    got, fn = _run_layer("cuda", torch.float32, "hip", weights, torch.from_numpy(g["voxels"]), torch.from_numpy(g["num_points"]),
                         torch.from_numpy(g["coords"]), torch.from_numpy(g["w"]), 64)
    assert fn == "PFNRadiusTrainFunctionBackward"            # the kernels, not the torch formulation
    assert tuple(got["d_linear_weight"].shape) == (64, 8)
    errs = {k: _rel(got[k], g[k]) for k in PROJECT_TOL}
    bounds = {k: max(PROJECT_TOL[k], 4 * float(g["f32_err." + k])) for k in PROJECT_TOL}
    print("fixture", {k: (f"{errs[k]:.2e}", f"{bounds[k]:.1e}") for k in errs})
    assert all(errs[k] <= bounds[k] for k in errs), (errs, bounds)


# (pillars, slots, channels, norm bias range).  (1, 2): the smallest BatchNorm accepts; (3, 127): the slot limit of the int8 argmax,
# two passes of the pillar-mean loop; (5000, 20): more than 1024 blocks x 4 waves, so the grid-stride loop and the 1024-partial
# reduction run; C = 16: lanes 16..63 idle; bias 2..4: relu(bn(0)) of the padded slots wins the max for some channels
CASES = [(1, 2, 64, (-0.3, 0.3)), (33, 5, 64, (-0.3, 0.3)), (3, 127, 64, (-0.3, 0.3)), (700, 60, 64, (-0.3, 0.3)),
         (5000, 20, 64, (-0.3, 0.3)), (700, 60, 16, (-0.3, 0.3)), (33, 5, 16, (-0.3, 0.3)), (33, 5, 64, (2.0, 4.0))]


@pytest.mark.parametrize("pillars,slots,channels,bias", CASES)
def test_radius_training_kernels_match_the_float64_formulation(pillars, slots, channels, bias):
    vox, num, coors = ragged_pillars(pillars, slots, seed=pillars * 131 + slots)
    assert float(vox[0, 0, 0]) == 0.0 and float(vox[0, 0, 1]) == 0.0 and int(num[0]) == slots          # the point on the sensor axis
    gen = torch.Generator().manual_seed(channels + slots)
    weights = dict(linear_weight=torch.empty(channels, 8).uniform_(-0.35, 0.35, generator=gen),
                   norm_weight=torch.empty(channels).uniform_(0.5, 1.5, generator=gen),
                   norm_bias=torch.empty(channels).uniform_(*bias, generator=gen))
    w = torch.randn(pillars, channels, generator=gen)
    ref, fn64 = _run_layer("cpu", torch.float64, "hip", weights, vox, num, coors, w, channels)
    f32, fn32 = _run_layer("cuda", torch.float32, "torch", weights, vox, num, coors, w, channels)
    got, fn = _run_layer("cuda", torch.float32, "hip", weights, vox, num, coors, w, channels)
    assert fn == "PFNRadiusTrainFunctionBackward" and fn32 != fn and fn64 != fn
    assert tuple(got["d_linear_weight"].shape) == (channels, 8)
    if bias[0] > 1 and pillars > 8:
        # the padded slots' value is the same for every pillar that has one and a lower bound of its output: a minimum that two
        # ragged pillars share (and that is positive) is that value -- the padded slot won there
        ragged = ref["out"][num < slots]
        lo = ragged.min(0).values
        assert bool((((ragged == lo).sum(0) >= 2) & (lo > 0)).any()), "no channel where a padded slot wins the max"
    errs = {k: _rel(got[k], ref[k]) for k in PROJECT_TOL}
    bounds = {k: max(PROJECT_TOL[k], 4 * _rel(f32[k], ref[k])) for k in PROJECT_TOL}
    print("case", (pillars, slots, channels, bias), {k: (f"{errs[k]:.2e}", f"{bounds[k]:.1e}") for k in errs})
    assert all(errs[k] <= bounds[k] for k in errs), (errs, bounds)


def test_radius_training_entry_points_with_no_pillars():
    """num_pillars == 0: the forward launches nothing (outputs untouched), the backward zero-fills the three gradients."""
    from second_amd import runtime as rt
    l = rt.lib()
    c = 64
    dev = "cuda"
    f = lambda n, v: torch.full((n,), v, dtype=torch.float32, device=dev)
    some = f(64, 1.0)
    ints = torch.zeros(16, dtype=torch.int32, device=dev)
    out, stats, arg = f(c, 7.0), f(c * 10 + 8, 7.0), torch.full((c,), 5, dtype=torch.int8, device=dev)
    rm, rv = f(c, 0.25), f(c, 0.5)
    ws = rt.workspace(l.sec_pfn_train_workspace_bytes(0, c), dev)
    rc = l.sec_pfn_radius_train_fwd(rt.ptr(some), rt.ptr(ints), rt.ptr(ints), 0, 60, 4, rt.ptr(some), rt.ptr(some), rt.ptr(some), 1e-3, 0.01,
                                    rt.ptr(rm), rt.ptr(rv), c, 0.25, 0.25, -49.875, -49.875, rt.ptr(out), rt.ptr(arg), rt.ptr(stats),
                                    rt.ptr(ws), ws.numel(), rt.stream())
    assert rc == 0
    dw, dg, db = f(8 * c + 4, float("nan")), f(c + 4, float("nan")), f(c + 4, float("nan"))     # four guard values behind each
    rc = l.sec_pfn_radius_train_bwd(rt.ptr(some), rt.ptr(ints), rt.ptr(ints), 0, 60, 4, rt.ptr(some), rt.ptr(some), rt.ptr(stats), c,
                                    0.25, 0.25, -49.875, -49.875, rt.ptr(some), rt.ptr(out), rt.ptr(arg), rt.ptr(dw), rt.ptr(dg), rt.ptr(db),
                                    rt.ptr(ws), ws.numel(), rt.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((stats == 7).all()) and bool((arg == 5).all()) and bool((rm == 0.25).all()) and bool((rv == 0.5).all())
    for t, n in ((dw, 8 * c), (dg, c), (db, c)):
        assert bool((t[:n] == 0).all()) and bool(torch.isnan(t[n:]).all())


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def reproducible_convs():
    """The trainer tests compare two executions of the same step (trainer against hand-assembled, captured against eager).  MIOpen's
    default convolution solvers are not reproducible run to run (7e-6 of a gradient's maximum in fp32 on this network), and at this
    geometry -- block 2 works on 2 x 10 x 10 cells -- one ReLU that flips on such a difference moves an element of a weight gradient by
    a percent (in bf16: tens of percent of whole tensors, eager against eager).  With torch.backends.cudnn.deterministic the dense
    segment, hand-written kernels included, was measured bit-reproducible, so the comparisons below test the code and not the noise."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _detector(seed=0):
    from second_amd import models
    torch.manual_seed(seed)
    return models.SecondDetector(small_cfg()).cuda()


def _args(det):
    return tuple(torch.from_numpy(a).cuda() for a in small_batch(det))


def _grads(det):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in det.named_parameters()}


def _assert_grads_agree(a, b, tol=1e-3):
    worst = ("", 0.0)
    for n in a:
        assert a[n] is not None and b[n] is not None, n
        err = float((a[n] - b[n]).abs().max()) / max(float(b[n].abs().max()), 1e-30)
        if err > worst[1]:
            worst = (n, err)
    print("worst gradient", worst)
    assert worst[1] <= tol, worst


def _learns(tr, args):
    losses = [float(tr.step(*args)[0]) for _ in range(6)]
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_multi_head_trainer_fp32_matches_the_hand_assembled_step_and_learns(reproducible_convs):
    from second_amd import models, ops
    from second_amd.training import MultiHeadDeviceTrainer
    det = _detector()
    hand = copy.deepcopy(det).train()
    names = [n for n, _ in det.named_parameters()]
    assert any(n.startswith("small_head.net.") for n in names) and any(n.startswith("large_head.") for n in names)
    assert "voxel_feature_extractor.pfn_layers.0.linear.weight" in names
    tr = MultiHeadDeviceTrainer(det, lr=1e-3)
    args = _args(det)
    pts, offs, gt, goffs, gcls = args
    loss, out6, labels = tr.forward_loss(*args)
    loss.backward()
    # the same computation by hand: module graph in training mode (the PFN layer on the same kernels), per-class targets, the loss
    cfg = hand.cfg
    begin = models.anchor_class_ranges(cfg, hand.feature_map_size)
    with torch.no_grad():
        vox = hand.voxel_generator.generate_device(pts, offs)
        lab2, reg2, imp2 = ops.assign_targets_per_class(hand.anchors, gt, goffs, gcls, begin, cfg["group_class_ids"], cfg["matched_thresholds"],
                                                        cfg["unmatched_thresholds"])
    feats = hand.voxel_feature_extractor(vox["voxels"], vox["num_points_per_voxel"], vox["coordinates"])
    assert type(feats.grad_fn).__name__ == "PFNRadiusTrainFunctionBackward"
    preds = hand._network_forward(feats, vox["coordinates"], 2)
    loss_cfg = dict(ops.LOSS_DEFAULTS, direction_offset=cfg["direction_offset"], num_class=cfg["num_class"], num_direction_bins=cfg["num_direction_bins"])
    loss2, out6b = ops.SecondLossFunction.apply(preds["cls_preds"], preds["box_preds"], preds["dir_cls_preds"], lab2, reg2, hand.anchors, imp2, loss_cfg)
    loss2.backward()
    assert torch.equal(labels, lab2)
    print("loss", float(loss.detach()), float(loss2.detach()))
    assert abs(float(loss.detach()) - float(loss2.detach())) <= 1e-4 * abs(float(loss2.detach()))
    ga, gb = _grads(det), _grads(hand)
    _assert_grads_agree(ga, gb)
    dead = [n for n, g in ga.items() if g is None or not torch.isfinite(g).all() or float(g.abs().max()) == 0.0]
    assert not dead, dead
    # every ground-truth class has positives inside its own anchor range, and no range holds another class's label
    lab, gc, go = labels.cpu().numpy(), gcls.cpu().numpy(), goffs.cpu().numpy()
    assert len(set(GT_CLASSES) & set(range(1, 6))) >= 2 and len(set(GT_CLASSES) & set(range(6, 11))) >= 2
    for f in range(2):
        for c in set(gc[go[f]:go[f + 1]].tolist()):
            assert (lab[f, begin[c - 1]:begin[c]] == c).any(), (f, c)
        for c in range(1, 11):
            assert set(np.unique(lab[f, begin[c - 1]:begin[c]]).tolist()) <= {-1, 0, c}
    for p in det.parameters():
        p.grad = None
    tr.bucket.zero_grad()
    _learns(tr, args)


def _unbiased_var(x):
    x = x.detach().float()
    return x.transpose(0, 1).reshape(x.shape[1], -1).var(dim=1, unbiased=True)


def test_multi_head_trainer_bf16_graphed_matches_eager_and_learns(reproducible_convs):
    from second_amd.training import MultiHeadDeviceTrainer
    det_g = _detector()
    det_e = copy.deepcopy(det_g)
    tr_g = MultiHeadDeviceTrainer(det_g, lr=1e-3, amp_dtype=torch.bfloat16)
    tr_e = MultiHeadDeviceTrainer(det_e, lr=1e-3, amp_dtype=torch.bfloat16)
    tr_e.graph_rpn = False
    assert tr_g.graph_rpn
    args = _args(det_g)
    res = []
    for tr in (tr_g, tr_e):
        loss, _, _ = tr.forward_loss(*args)
        loss.backward()
        res.append((float(loss.detach()), _grads(tr.det)))
        for p in tr.det.parameters():
            p.grad = None
        tr.bucket.zero_grad()
    assert tr_g._graphed_rpn is not None and tr_g._graphed_rpn[1] is not None, "the dense segment was not captured"
    assert tr_e._graphed_rpn is None
    print("loss graphed / eager", res[0][0], res[1][0])
    assert abs(res[0][0] - res[1][0]) <= 1e-4 * abs(res[1][0])
    _assert_grads_agree(res[0][1], res[1][1])
    # one step: counters advance by exactly one; the tower's running_var moves with momentum 0.1, the trunk's with 0.01
    tower, trunk = "small_head.net.1", "rpn.blocks.0.2"
    seen = {}
    mods_e = dict(det_e.named_modules())
    hooks = [mods_e[n].register_forward_hook(lambda m, i, o, n=n: seen.__setitem__(n, _unbiased_var(i[0]))) for n in (tower, trunk)]
    counters = [tower, "small_head.net.4", "small_head.net.7", "voxel_feature_extractor.pfn_layers.0.norm", trunk]
    for tr in (tr_g, tr_e):
        mods = dict(tr.det.named_modules())
        before = {n: (int(mods[n].num_batches_tracked), mods[n].running_var.clone()) for n in counters}
        tr.step(*args)
        torch.cuda.synchronize()
        for n in counters:
            assert int(mods[n].num_batches_tracked) == before[n][0] + 1, (n, tr.graph_rpn)
        tr.rv_before = before
    for h in hooks:
        h.remove()
    mods_g = dict(det_g.named_modules())
    for n, mom in ((tower, 0.1), (trunk, 0.01)):
        assert mods_e[n].momentum == mom
        want = (1 - mom) * tr_e.rv_before[n][1] + mom * seen[n]
        other = (1 - (0.11 - mom)) * tr_e.rv_before[n][1] + (0.11 - mom) * seen[n]           # what the other layer's momentum would give
        err, err_other = _rel(mods_e[n].running_var, want), _rel(mods_e[n].running_var, other)
        print(n, "running_var vs momentum", mom, err, "vs the other momentum", err_other)
        assert err <= 1e-3 and err_other > 10 * err
        assert _rel(mods_g[n].running_var, mods_e[n].running_var) <= 1e-3                    # the replayed segment moves them alike
    _learns(tr_g, args)
