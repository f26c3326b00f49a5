"""Training-mode ``net(example)`` behind compat.accelerate_model (second_amd/dropin_train.py): the reference's training loop
(second/pytorch/train.py:306-330) on a network object shaped like ``build_network``'s (tests/reference_standin.py), served from
two hipGraph replays per step.

  * captured static-capacity step == the same step launched eagerly with dynamic shapes (same kernels, same precision): loss
    scalars to 1e-4, every parameter gradient to 1e-3 of its maximum, per-anchor tensors, BatchNorm running statistics;
  * against the un-accelerated fp32 module graph (the reference's own arithmetic): 16-bit-feature bounds, stated below;
  * the loop itself: clip_grad_norm_ + a torch optimizer + zero_grad on the REFERENCE's parameters, loss goes down, weights move,
    gradient accumulation and the non-None ``.grad`` cases, backward of a stale forward refused."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _net(seed=0):
    from reference_standin import build_voxelnet
    from second_amd.models import CAR_FHD
    torch.manual_seed(seed)
    return build_voxelnet(CAR_FHD).cuda().train()


def _example(net, seeds=(0, 1), npts=6000, nvox=5000):
    from reference_standin import train_example_of
    from second_amd import synthetic as syn
    clouds = [syn.syn_kitti_cloud(s, num_points=npts, num_voxels=nvox) for s in seeds]
    boxes = [syn.syn_kitti_boxes(s, 10) for s in seeds]
    return train_example_of(net, clouds, boxes, torch.device("cuda"))


def _grads(net):
    return {n: p.grad.detach().float().clone() for n, p in net.named_parameters() if p.grad is not None}


def test_fused_training_forward_backward_equals_the_eager_form_of_the_same_step():
    from second_amd import compat
    net = _net()
    ref = _net()
    ref.load_state_dict(net.state_dict())
    ex = _example(net)
    compat.accelerate_model(net, train_dtype=torch.bfloat16)
    compat.accelerate_model(ref, train_dtype=torch.bfloat16)
    out = net(ex)
    eng = net._second_amd_engine
    assert eng.stats["train_calls"] == 1 and eng.stats["original_calls"] == 0, eng.stats
    assert out["loss"].requires_grad and out["loss"].dim() == 0
    out["loss"].mean().backward()
    ref._second_amd_engine._accepts_training(ex)
    eo = ref._second_amd_engine.trainer.eager(ex)
    eo["loss"].mean().backward()
    torch.cuda.synchronize()
    for k in ("loss", "cls_loss_reduced", "loc_loss_reduced", "dir_loss_reduced", "cls_pos_loss", "cls_neg_loss"):
        a, b = float(out[k].detach()), float(eo[k].detach())
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (k, a, b)
    for k in ("cls_preds", "cls_loss", "loc_loss"):
        assert out[k].shape == eo[k].shape
        torch.testing.assert_close(out[k].float(), eo[k].float(), rtol=1e-3, atol=1e-4 * float(eo[k].abs().max()) + 1e-7, msg=k)
    assert out["cls_preds"].shape == (2, 2, 200, 176, 1) and out["cls_loss"].shape == (2, 70400, 1) and out["loc_loss"].shape == (2, 70400, 7)
    assert torch.equal(out["cared"], ex["labels"] >= 0)
    ga, gb = _grads(net), _grads(ref)
    assert set(ga) == set(gb) == {n for n, p in net.named_parameters() if p.requires_grad}
    for n in ga:
        err = (ga[n] - gb[n]).abs().max().item()
        assert err <= 1e-3 * gb[n].abs().max().item() + 1e-9, (n, err, gb[n].abs().max().item())
    # BatchNorm running statistics moved on the reference's own buffers, identically
    for (n, a), (_, b) in zip(net.named_buffers(), ref.named_buffers()):
        if "running_" in n:
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6, msg=n)
        elif "num_batches" in n:
            assert int(a) == int(b) == 1, (n, int(a), int(b))


def test_fused_training_against_the_fp32_module_graph():
    """The un-accelerated forward of the same object (three modules per sparse layer, .dense(), torch RPN, torch loss) is fp32; the
    captured step keeps 16-bit (bf16: 8 significant bits) features.  What can be bounded between the two (tools/dropin_train_probe.py
    prints the statistics): loss scalars 3 %; head logits L2-relative 8 % (measured 4.3 %; median |difference| 5e-4 on values of rms
    0.38, isolated anchors up to 0.9 where a rounding flipped a ReLU mask 20 train-mode-BatchNorm layers up); gradients of the three
    heads 10 % of their maximum (measured 0.2-6 %).  Below the heads every gradient passes BatchNorm backward, which subtracts the
    mean gradient -- at initialisation ~140 k negative anchors push every pixel the same way, the surviving residual is a small
    difference of large terms and the 8-bit rounding of dY is amplified: 20-50 % L2-relative against fp32 for ANY bf16 chain (torch
    autocast shows the same, tests/test_gpu_train_dense.py::test_rpn_forward_mixed_hip_vs_fp32_and_torch_autocast), so the bound there is on direction, cosine >= 0.8
    (measured 0.86-0.99).  Exactness of the captured step itself is the previous test's job (same kernels, 1e-3).  What pins the
    16-bit gradients below the heads is tests/test_gpu_train_step_audit.py: every node of a real step against fp64 on the inputs the
    step itself gave it, where no ReLU flip compounds; the cosine here only says that the two chains agree in direction."""
    from second_amd import compat
    net = _net(1)
    ex = _example(net, seeds=(2, 3))
    plain = _net(1)
    plain.load_state_dict(net.state_dict())
    compat.accelerate_model(net, train_dtype=torch.bfloat16)
    out = net(ex)
    out["loss"].backward()
    po = plain(ex)
    po["loss"].backward()
    torch.cuda.synchronize()
    for k in ("loss", "cls_loss_reduced", "loc_loss_reduced", "dir_loss_reduced"):
        a, b = float(out[k].detach()), float(po[k].detach())
        assert abs(a - b) <= 3e-2 * max(1.0, abs(b)), (k, a, b)
    a, b = out["cls_preds"].reshape(-1).float(), po["cls_preds"].reshape(-1).float().detach()
    assert ((a - b).norm() / b.norm()).item() < 0.08
    assert (a - b).abs().median().item() < 5e-3
    ga, gb = _grads(net), _grads(plain)
    assert set(ga) == set(gb)
    for n in gb:
        if n.startswith("rpn.conv_"):
            rel = (ga[n] - gb[n]).abs().max().item() / (gb[n].abs().max().item() + 1e-20)
            assert rel < 0.1, (n, rel)
        else:
            cos = torch.nn.functional.cosine_similarity(ga[n].reshape(-1), gb[n].reshape(-1), dim=0).item()
            assert cos > 0.8, (n, cos)


def test_reference_training_loop_runs_on_the_reference_parameters():
    """train.py:306-330 verbatim in shape: forward, mean, backward, clip, optimizer step, zero_grad -- torch.optim.Adam on the
    network's own parameters.  The loss falls on a repeated batch; accumulate semantics hold when zero_grad is skipped."""
    from second_amd import compat
    net = _net(2)
    ex = _example(net, seeds=(4, 5))
    compat.accelerate_model(net, train_dtype=torch.bfloat16)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    w0 = net.rpn.conv_cls.weight.detach().clone()
    losses = []
    for step in range(12):
        ret = net(ex)
        loss = ret["loss"].mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 10.0)
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    eng = net._second_amd_engine
    assert eng.stats["train_calls"] == 12 and eng.stats["original_calls"] == 0 and eng.stats["train_captures"] == 1, eng.stats
    assert losses[-1] < 0.7 * losses[0], losses
    assert not torch.equal(w0, net.rpn.conv_cls.weight)
    assert int(net.rpn.blocks[0][2].num_batches_tracked) == 12
    # accumulation: two backward passes without zero_grad = twice the gradient
    net(ex)["loss"].backward()
    g1 = _grads(net)
    net(ex)["loss"].backward()
    g2 = _grads(net)
    for n in g1:
        torch.testing.assert_close(g2[n], 2 * g1[n], rtol=2e-2, atol=2e-3 * float(g1[n].abs().max()) + 1e-9, msg=n)
    # a gradient tensor of the caller's own (not the bucket view) is added to, not replaced
    opt.zero_grad()
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    net(ex)["loss"].backward()
    g3 = _grads(net)
    for n in g1:
        torch.testing.assert_close(g3[n] - 1.0, g1[n], rtol=2e-2, atol=2e-3 * float(g1[n].abs().max()) + 1e-6, msg=n)
    # backward of an older forward is refused (the captured step keeps the latest activations only)
    opt.zero_grad()
    old = net(ex)["loss"]
    net(ex)
    with pytest.raises(RuntimeError, match="older net"):
        old.backward()


def test_training_calls_grow_capacity_and_eval_mode_still_uses_the_inference_graph():
    from second_amd import compat
    net = _net(3)
    small = _example(net, seeds=(0, 1), npts=3000, nvox=2500)
    big = _example(net, seeds=(0, 1), npts=17000, nvox=16000)
    compat.accelerate_model(net, train_dtype=torch.bfloat16)
    net(small)["loss"].backward()
    net(big)["loss"].backward()
    eng = net._second_amd_engine
    assert eng.stats["train_captures"] + eng.stats["train_overflow_recaptures"] >= 2 and eng.stats["original_calls"] == 0, eng.stats
    net.eval()
    with torch.no_grad():
        res = net({k: v for k, v in big.items() if k not in ("labels", "reg_targets", "importance")})
    assert len(res) == 2 and res[0]["box3d_lidar"].shape[1] == 7 and eng.stats["fused_calls"] == 1
    net.train()
    net(small)["loss"].backward()
    assert eng.stats["original_calls"] == 0


def test_training_outside_the_captured_step_keeps_the_original_forward():
    from second_amd import compat
    net = _net(4)
    ex = _example(net)
    net._loss_norm_type.name = "NormByNumExamples"
    compat.accelerate_model(net, train_dtype=torch.bfloat16)
    out = net(ex)                                           # the stand-in's own torch loss (NormByNumPositives formula: only the routing is tested)
    eng = net._second_amd_engine
    assert eng.stats["original_calls"] == 1 and "loss_norm_type" in eng.stats["train_fallback_reason"]
    assert out["loss"].requires_grad
    plain = _net(4)
    compat.accelerate_model(plain)                          # no train_dtype: training stays on the original forward
    plain(ex)
    assert plain._second_amd_engine.stats["original_calls"] == 1


def test_fp16_features_with_a_scaled_loss():
    """``train_dtype=torch.float16`` and a caller that scales its loss (apex ``amp.scale_loss``, train.py:318-320): the factor arrives at
    the backward graph as the gradient of ``loss`` (a device scalar) and every parameter gradient carries it."""
    from second_amd import compat
    net = _net(5)
    ex = _example(net, seeds=(6, 7))
    compat.accelerate_model(net, train_dtype=torch.float16)
    net(ex)["loss"].backward()
    g1 = _grads(net)
    for p in net.parameters():
        p.grad = None
    (net(ex)["loss"] * 64.0).backward()
    g64 = _grads(net)
    eng = net._second_amd_engine
    assert eng.stats["train_calls"] == 2 and eng.stats["original_calls"] == 0 and eng.trainer.dtype == torch.float16
    for n in g1:
        assert torch.isfinite(g64[n]).all(), n
        ref = 64.0 * g1[n]
        # (the second forward saw BatchNorm statistics moved once by the first: a 1 % effect; fp16 rounding of the scaled gradients on top)
        assert (g64[n] - ref).abs().max().item() <= 0.1 * ref.abs().max().item() + 1e-6, n
