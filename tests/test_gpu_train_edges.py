"""-m gpu: the kernels of csrc/train.hip against the float64 references of tests/train_ref_helpers.py (pinned to the reference's own
fixtures by tests/test_train_ref_host.py) where tests/test_gpu_train.py does not reach: ground truth beyond one LDS chunk of 256
boxes, every branch of the loss's hyper-parameters, the unrolled loop of the bias-gradient reduction, grid-stride second trips of
the flat AdamW.  Tolerances are the project's own (test_gpu_train.py, test_gpu_train_dense.py).  Yardstick: the loss reference
evaluated in fp32 on the CPU differs from float64 on these inputs by at most 2.7e-6 relative in the scalars and 1.3e-6 of the
largest entry in the gradients (test_train_ref_host.py keeps four times that inside the tolerances)."""
import ctypes

import numpy as np
import pytest
import torch

import train_ref_helpers as H

pytestmark = pytest.mark.gpu

SEEDS = (0, 1)            # tests/test_train_ref_host.py::test_lattice_case_meets_its_own_conditions runs the same ones


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


@pytest.fixture(scope="module")
def lattice():
    return {s: H.lattice_case(s) for s in SEEDS}


def _flat(c):
    offs = np.cumsum([0] + [len(g) for g in c["gt"]]).astype(np.int32)
    return (dev(c["anchors"]), dev(np.concatenate(c["gt"])), dev(offs), dev(np.concatenate(c["classes"])), dev(np.concatenate(c["importance"])))


def _compare_assignment(got, want_frames):
    labels, targets, importance = (t.cpu().numpy() for t in got)
    for f, (l, t, i) in enumerate(want_frames):
        np.testing.assert_array_equal(labels[f], l, err_msg=f"labels of frame {f}")
        np.testing.assert_array_equal(importance[f], i, err_msg=f"importance of frame {f}")
        np.testing.assert_allclose(targets[f], t, rtol=1e-5, atol=2e-6, err_msg=f"targets of frame {f}")


# ----------------------------------------------------------------------------------------------------------- target assignment
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("thresholds", H.LATTICE_THRESHOLDS)
def test_assign_targets_beyond_one_lds_chunk(ops, lattice, seed, thresholds):
    """874 anchors (under four workgroups, no multiple of 256) against frames of 300, 256, 257, 0 and 1 ground-truth boxes with
    classes and importance: labels and importance equal the float64 matching, box targets within the fixture test's tolerance."""
    c = lattice[seed]
    anchors, gt, offs, cls, imp = _flat(c)
    matched, unmatched = thresholds
    got = ops.assign_targets(anchors, gt, offs, matched, unmatched, gt_classes=cls, gt_importance=imp)
    want = [H.assign_ref(c["anchors"], g, matched, unmatched, k, i)[:3] for g, k, i in zip(c["gt"], c["classes"], c["importance"])]
    _compare_assignment(got, want)
    lab = got[0].cpu().numpy()
    assert (lab[3] == 0).all() and set(np.unique(lab[0]).tolist()) == {-1, 0, 1, 2, 3}


PER_CLASS_MATCHED, PER_CLASS_UNMATCHED = [0.6, 0.5, 0.5], [0.45, 0.375, 0.375]


@pytest.mark.parametrize("begins", [(0, 301, 301, 874), (0, 130, 301, 874)], ids=["empty_range", "three_ranges"])
@pytest.mark.parametrize("ids", [[1, 2, 3], [0, 0, 0]], ids=["per_class", "all"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "anchors_mask"])
def test_assign_targets_per_class_beyond_one_lds_chunk(ops, lattice, begins, ids, masked):
    """Anchor ranges with unaligned begins (one of them empty in one variant), class-filtered ground truth with fewer than ten boxes
    of class 2 among 300 (some past index 256), a frame without class 3, per-range thresholds; with and without an anchors mask
    that drops about 30 % of the entries."""
    c = lattice[1]
    anchors, gt, offs, cls, imp = _flat(c)
    mask = None
    if masked:
        mask = np.random.default_rng(7).random((len(c["gt"]), len(c["anchors"]))) >= 0.3
        assert 0.25 < 1.0 - mask.mean() < 0.35
    got = ops.assign_targets_per_class(anchors, gt, offs, cls, list(begins), ids, PER_CLASS_MATCHED, PER_CLASS_UNMATCHED, gt_importance=imp,
                                       anchors_mask=None if mask is None else dev(mask))
    want = [H.assign_per_class_ref(c["anchors"], g, k, list(begins), ids, PER_CLASS_MATCHED, PER_CLASS_UNMATCHED, gt_importance=i,
                                   mask=None if mask is None else mask[f])
            for f, (g, k, i) in enumerate(zip(c["gt"], c["classes"], c["importance"]))]
    _compare_assignment(got, want)
    if not masked and ids[0] and begins[1] != begins[2]:
        lab = got[0].cpu().numpy()
        assert (lab[0, begins[1]:begins[2]] == 2).any() and (lab[1, begins[2]:] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------ loss
LOSS_CFGS = {"defaults": {}, "nondefault": H.LOSS_NONDEFAULT, "gamma0": dict(gamma=0.0)}


def _check_scalars(got, want):
    """rtol 1e-4 (test_gpu_train.py); a term whose reference is exactly zero may be off by 1e-7."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = np.where(want == 0, 1e-7, 1e-4 * np.abs(want))
    assert np.all(np.abs(got - want) <= tol), (got, want)


def _check_grad(name, got, want):
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6 * np.abs(want).max() + 1e-9, err_msg=name)


def _run_loss(ops, c, nc, bins, cfg):
    out6, d_cls, d_box, d_dir = ops.second_loss_raw(dev(c["cls"]), dev(c["box"]), None if bins == 0 else dev(c["dir"]), dev(c["labels"]),
                                                    dev(c["reg"]), dev(c["anchors"]), dev(c["importance"]), **cfg)
    ref6, r_cls, r_box, r_dir = H.loss_ref(c["cls"], c["box"], c["dir"], c["labels"], c["reg"], c["anchors"], c["importance"],
                                           num_class=nc, num_direction_bins=bins, **cfg)
    _check_scalars(out6.cpu().numpy(), ref6)
    _check_grad("cls", d_cls.cpu().numpy(), r_cls)
    _check_grad("box", d_box.cpu().numpy(), r_box)
    if bins:
        _check_grad("dir", d_dir.cpu().numpy(), r_dir)
    else:
        assert d_dir is None and float(out6[3]) == 0.0
    return ref6


@pytest.mark.parametrize("cfg", list(LOSS_CFGS), ids=list(LOSS_CFGS))
@pytest.mark.parametrize("shape", [(37, 1, 2), (1000, 3, 4), (1000, 1, 0)], ids=["n37_c1_b2", "n1000_c3_b4", "n1000_c1_nodir"])
def test_second_loss_hyper_parameters_and_shapes(ops, cfg, shape):
    """sec_second_loss_f32 against standin_loss in float64 on the same fp32 inputs: focal gamma 2 / 1.5 (powf, value and
    derivative) / 0, class weights, code weights, sin factor 2, four direction bins with an offset, no direction head; 37 anchors
    (fewer than the 64 count chunks) and 1000 (no multiple of 256); frame 1 without a positive anchor."""
    n, nc, bins = shape
    cfg = LOSS_CFGS[cfg]
    c = H.loss_case(11, 3, n, nc, bins, direction_offset=cfg.get("direction_offset", 0.0))
    assert not (c["labels"][1] > 0).any() and (c["labels"][0] > 0).any()
    ref6 = _run_loss(ops, c, nc, bins, cfg)
    assert ref6[1] > 0 and ref6[2] > 0 and (bins == 0 or ref6[3] > 0)


def test_second_loss_all_anchors_dont_care(ops):
    """Every label -1: all six scalars and all gradients are zero, nothing divides by a zero count."""
    c = H.loss_case(3, 3, 1000, 3, 4, all_dont_care=True)
    ref6 = _run_loss(ops, c, 3, 4, H.LOSS_NONDEFAULT)
    assert np.all(ref6 == 0)


# ----------------------------------------------------------------------------------------------------------- stacked-heads loss
def _heads_case(b, h, w, bins, dtype, cfg):
    """A 16-bit [B, H, W, 64] head tensor (box [2 * 7] | cls [2] | dir [2 * bins] | padding filled with noise the kernel must ignore)
    and the three-tensor view of its VALUES: anchor n = a * H * W + pixel."""
    hw, a = h * w, 2
    n = a * hw
    c = H.loss_case(100 + b + bins, b, n, 1, bins, direction_offset=cfg.get("direction_offset", 0.0))
    y = torch.randn(b, hw, 64, generator=torch.Generator().manual_seed(b))
    to_y = lambda x, code: torch.from_numpy(x).reshape(b, a, hw, code).permute(0, 2, 1, 3).reshape(b, hw, a * code)
    y[..., :14], y[..., 14:16] = to_y(c["box"], 7), to_y(c["cls"], 1)
    if bins:
        y[..., 16:16 + a * bins] = to_y(c["dir"], bins)
    y = y.to(dtype).reshape(b, h, w, 64).contiguous()
    back = lambda c0, code: y.float().reshape(b, hw, 64)[..., c0:c0 + a * code].reshape(b, hw, a, code).permute(0, 2, 1, 3).reshape(b, n, code).numpy()
    c["box"], c["cls"] = back(0, 7), back(14, 1)
    c["dir"] = back(16, bins) if bins else None
    return c, y


@pytest.mark.parametrize("dtype,grad_loss", [(torch.bfloat16, 3.0), (torch.float16, 512.0)], ids=["bf16", "fp16_scale512"])
@pytest.mark.parametrize("bins", [2, 0])
@pytest.mark.parametrize("cfg", ["defaults", "nondefault"])
@pytest.mark.parametrize("shape", [(2, 24, 20), (4, 64, 60)], ids=["b2_24x20", "b4_64x60"])
def test_heads_loss_against_the_float64_loss(dtype, grad_loss, bins, cfg, shape):
    """sec_heads_loss_fwd / sec_heads_loss_bwd called directly.  b=4, 64x60 is 15 workgroups x 4 frames = 60 partial rows, the
    smallest shape that enters the eight-loads-in-flight loop of k_heads_bias_final (4 partials at b=2, 24x20).  Scalars: the loss
    tolerances.  d_heads: g * reference rounded once to the dtype (relative 2^-8 bf16, 2^-10 fp16, plus 1e-6 of the largest
    entry, plus 2^-24 for fp16 subnormals).  d_bias: the float64 column sums of the RETURNED d_heads within 1e-5 of the column's
    absolute sum.  Channels behind the heads are zero; two calls give the same bits."""
    from second_amd import ops, runtime as rt
    b, h, w = shape
    cfg = LOSS_CFGS[cfg]
    c, y = _heads_case(b, h, w, bins, dtype, cfg)
    n, tot = 2 * h * w, 2 * (7 + 1 + bins)
    assert (b * ((h * w + 255) // 256) >= 58) == (shape == (4, 64, 60))
    y = y.cuda()
    labels, reg, anchors, imp = dev(c["labels"]), dev(c["reg"]), dev(c["anchors"]), dev(c["importance"])
    assert labels.shape == (b, n) and reg.shape == (b, n, 7) and anchors.shape == (n, 7) and imp.shape == (b, n) and y.numel() == b * h * w * 64
    params = ops._loss_params(dict(H.LOSS_DEFAULTS, **cfg))
    l = rt.lib()
    g = torch.tensor([grad_loss], dtype=torch.float32, device="cuda")

    def run():
        out6 = torch.empty(6, device="cuda")
        d_heads = torch.full_like(y, float("nan"))
        d_bias = torch.full((64,), float("nan"), device="cuda")
        ws = rt.workspace(l.sec_heads_loss_workspace_bytes(b, h, w, 2), y.device)
        rt.check(l.sec_heads_loss_fwd(rt.ptr(y), rt.dtype_code(dtype), b, h, w, 64, 2, 1, bins, rt.ptr(labels), rt.ptr(reg), rt.ptr(anchors),
                                      rt.ptr(imp), params, rt.ptr(out6), rt.ptr(ws), ws.numel(), rt.stream()), "sec_heads_loss_fwd")
        ws2 = rt.workspace(l.sec_heads_loss_workspace_bytes(b, h, w, 2), y.device)
        rt.check(l.sec_heads_loss_bwd(rt.ptr(y), rt.dtype_code(dtype), b, h, w, 64, 2, 1, bins, rt.ptr(labels), rt.ptr(reg), rt.ptr(anchors),
                                      rt.ptr(imp), params, rt.ptr(g), rt.ptr(d_heads), rt.ptr(d_bias), rt.ptr(ws2), ws2.numel(), 0, rt.stream()),
                 "sec_heads_loss_bwd")
        torch.cuda.synchronize()
        return out6.cpu(), d_heads.cpu(), d_bias.cpu()

    out6, d_heads, d_bias = run()
    ref6, r_cls, r_box, r_dir = H.loss_ref(c["cls"], c["box"], c["dir"], c["labels"], c["reg"], c["anchors"], c["importance"],
                                           num_class=1, num_direction_bins=bins, **cfg)
    _check_scalars(out6.numpy(), ref6)
    # the reference gradient in the layout of y
    to_y = lambda x, code: x.reshape(b, 2, h * w, code).transpose(0, 2, 1, 3).reshape(b, h * w, 2 * code)
    want = np.zeros((b, h * w, 64))
    want[..., :14], want[..., 14:16] = to_y(r_box, 7), to_y(r_cls, 1)
    if bins:
        want[..., 16:16 + 2 * bins] = to_y(r_dir, bins)
    want *= grad_loss
    got = d_heads.double().numpy().reshape(b, h * w, 64)
    rel, sub = (2.0 ** -8, 0.0) if dtype == torch.bfloat16 else (2.0 ** -10, 2.0 ** -24)
    err = np.abs(got - want)
    tol = rel * np.abs(want) + 1e-6 * np.abs(want).max() + sub
    assert np.all(err <= tol), (float((err - tol).max()), np.unravel_index(np.argmax(err - tol), err.shape))
    assert np.all(got[..., tot:] == 0) and np.abs(got[..., :tot]).max() > 0
    for k0, k1 in ((0, 14), (14, 16)) + (((16, tot),) if bins else ()):
        assert (got[0, :, k0:k1] != 0).any(), (k0, k1)                       # every head receives a gradient (frame 1 has no positive)
    cols, mass = got.sum((0, 1)), np.abs(got).sum((0, 1))
    db = d_bias.double().numpy()
    assert np.all(np.abs(db - cols) <= 1e-5 * mass), (np.abs(db - cols) / np.maximum(mass, 1e-300)).max()
    assert np.all(db[tot:] == 0)
    again = run()
    assert torch.equal(out6, again[0]) and torch.equal(d_heads.view(torch.int16), again[1].view(torch.int16)) and torch.equal(d_bias, again[2])


# ----------------------------------------------------------------------------------------------------------------- flat AdamW
ADAM_N = 2048 * 256 * 4 + 1234      # past one trip of both grid-stride loops (512 and 2048 workgroups of 256 threads), odd tail
_f32 = lambda v: float(np.float32(v))


def _adam_steps(n, scales, lr, wd, max_norm, betas=(0.9, 0.99), eps=1e-8, seed=0):
    from second_amd.training import FlatAdamW
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    param = torch.nn.Parameter(p0.clone().cuda())
    grad = torch.zeros(n, device="cuda")
    opt = FlatAdamW([param], grad, lr, wd, betas=betas, eps=eps, max_grad_norm=max_norm)
    p, m, v = p0.double().numpy(), np.zeros(n), np.zeros(n)
    clipped = []
    for step, scale in enumerate(scales, 1):
        gr = torch.randn(n, generator=g) * scale
        grad.copy_(gr)
        opt.step()
        torch.cuda.synchronize()
        # the kernel receives the hyper-parameters as fp32: the reference computes in float64 on those values
        p, m, v, norm = H.adamw_ref(p, m, v, gr.double().numpy(), step, _f32(lr), _f32(betas[0]), _f32(betas[1]), _f32(eps), _f32(wd), _f32(max_norm))
        clipped.append(max_norm > 0 and norm > max_norm)
        state = opt.state.cpu().numpy()
        assert abs(float(state[0]) - norm) <= 1e-5 * norm and state[1] == step and state[2] == 0, (state, norm)
        np.testing.assert_allclose(param.detach().cpu().numpy(), p, rtol=2e-6, atol=2e-7, err_msg=f"step {step}")
        assert param.data_ptr() == opt.flat.data_ptr()
    return clipped, np.abs(p - p0.double().numpy())


def test_flat_adamw_second_grid_stride_trip_with_and_without_clipping():
    """Three steps of FlatAdamW (sec_flat_adamw_dev_f32) on 2 098 386 elements against the float64 formula: gradient norms of about
    1.4, 720 and 5.8 around max_grad_norm = 10."""
    clipped, moved = _adam_steps(ADAM_N, (0.001, 0.5, 0.004), 3e-3, 0.01, 10.0)
    assert clipped == [False, True, False]
    assert moved[-1234:].min() > 0 and moved[ADAM_N // 2:].min() > 0          # the tail moved too


def test_flat_adamw_without_clipping_and_without_weight_decay():
    """max_grad_norm = 0 switches the clipping off (the norm of 720 is still reported), weight_decay = 0."""
    clipped, _ = _adam_steps(ADAM_N, (0.5, 0.002), 1e-3, 0.0, 0.0, seed=1)
    assert clipped == [False, False]


def test_flat_adamw_host_arguments_equal_device_arguments():
    """sec_flat_adamw_f32 (hyper-parameters by value) and sec_flat_adamw_dev_f32 (the same six values in device memory) leave
    identical bits in param, exp_avg, exp_avg_sq and state."""
    from second_amd import runtime as rt
    l = rt.lib()
    n = 300017
    hyper = (3e-3, 0.9, 0.99, 1e-8, 0.01, 10.0)
    g = torch.Generator().manual_seed(2)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g).cuda() * s for s in (0.001, 0.5)]
    res = []
    for form in ("host", "dev"):
        p, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        state = torch.zeros(4, device="cuda")
        ws = torch.zeros(l.sec_flat_adamw_workspace_bytes(), dtype=torch.uint8, device="cuda")
        h6 = torch.tensor(hyper, dtype=torch.float32).cuda()
        for gr in grads:
            if form == "host":
                rc = l.sec_flat_adamw_f32(rt.ptr(p), rt.ptr(gr), rt.ptr(m), rt.ptr(v), n, *[ctypes.c_float(x) for x in hyper], rt.ptr(state), None,
                                          rt.ptr(ws), ws.numel(), rt.stream())
            else:
                rc = l.sec_flat_adamw_dev_f32(rt.ptr(p), rt.ptr(gr), rt.ptr(m), rt.ptr(v), n, rt.ptr(h6), rt.ptr(state), None, rt.ptr(ws),
                                              ws.numel(), rt.stream())
            rt.check(rc, "sec_flat_adamw " + form)
        torch.cuda.synchronize()
        res.append((p.cpu(), m.cpu(), v.cpu(), state.cpu()))
    for a, b, name in zip(res[0], res[1], ("param", "exp_avg", "exp_avg_sq", "state")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert res[0][3][1] == 2 and not torch.equal(res[0][0], p0)
