"""-m gpu: the dense RPN TRAINING kernels (csrc/dense_train.hip and the forward / data gradient on k_conv2d_halo_reg) element by element
against the fp64 references and per-element bounds of tests/dense_train_ref_helpers.py (derived there; tests/test_dense_train_ref_host.py
shows on the CPU that they catch a lost pixel, a missing row end or image wrap, mirrored taps, a transposed result, a wrong pitch,
biased running variance, statistics over dead rows, a mask from the stored z and swapped sums).  Operands are seeded on the CPU and
rounded to the dtype first, the reference sees the rounded values, no element is excluded.

  A  3x3 and one-tap weight gradient at small ragged shapes, both forms forced: gamma_n * sum |x||dy| per element, run twice
  B  the same kernels on small integers, where fp32 is exact in any order: np.array_equal -- the small shapes, the automatic switch to
     the row form (159 999 / 160 000 pixels), the re-slicing of the tap form (692 224 pixels), the car.fhd training shape
  C  Conv3x3Function, ConvTranspose1x1Function, Heads1x1Function end to end at (2, 19, 23)
  D  conv2d_pack_weight_train == the separate packs, zero block included
  E  BatchNorm + ReLU forward / backward: the small path, the switch to the three-launch path (131 072 / 131 073 rows), the
     offset-mean case, static capacity with NaN behind the live rows, BatchNormReluFunction on [N, C] rows

Largest error / bound reached, always against the fp64 reference (test_report_ratios of either file prints them; bf16 / fp16):
                                   numpy restatement (CPU)     MI355X
  wgrad 3x3, tap form              0.099 / 0.241               0.072 / 0.119
  wgrad 3x3, row form              0.099 / 0.241               0.072 / 0.119
  wgrad 1x1, cout 128              0.001 / 0.002               0.002 / 0.002
  wgrad 1x1, cout 64 (dyc form)    0.001 / 0.001               0.002 / 0.002
  BatchNorm mean                   0.069 / 0.069               0.069 / 0.069
  BatchNorm invstd                 0.169 / 0.179               0.169 / 0.179
  BatchNorm running mean / var     0.613 / 0.516, 0.466 / 0.456    0.613 / 0.516, 0.466 / 0.457
  BatchNorm dbeta, dgamma          0.007 / 0.017, 0.070 / 0.064    0.007 / 0.017, 0.070 / 0.064
  BatchNorm z, dy                  0.996 / 0.995, 0.995 / 0.994    0.996 / 0.995, 0.995 / 0.994
  Conv3x3Function y, dx, dW        --                          0.853 / 0.485, 0.860 / 0.515, 0.002 / 0.002
  ConvTranspose1x1Function         --                          0.988 / 0.928, 0.984 / 0.931, 0.001 / 0.001
  Heads1x1Function y, dx, dW, db   --                          0.977 / 0.952, 0.991 / 0.965, 0.001 / 0.001, 0.0001 / 0.0001
(The 16-bit outputs sit just under 1 by construction: the bound is the half-ulp of the store plus the small accumulation term, and
among thousands of elements one lands next to a rounding midpoint.)  Every integer case: 0 differing elements.
Wall time of this file on the MI355X: 23 s for 139 tests (slowest: 1.5 s, BatchNorm at 131 072 x 256), reference computation included.
"""
import numpy as np
import pytest
import torch

import dense_train_ref_helpers as H

pytestmark = pytest.mark.gpu

KINDS = {"bf16": torch.bfloat16, "fp16": torch.float16}
RATIOS = {}
_cache = {}


def note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


def nchw(a, dtype):
    """[B,H,W,C] numpy -> the channels_last [B,C,H,W] device tensor over the same memory order."""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype).permute(0, 3, 1, 2)


def nhwc_np(t):
    return t.detach().permute(0, 2, 3, 1).float().cpu().numpy()


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def set_form(monkeypatch, form):
    if form is None:
        monkeypatch.delenv("SEC_WGRAD_ROW", raising=False)
    else:
        monkeypatch.setenv("SEC_WGRAD_ROW", "1" if form == "row" else "0")


# ------------------------------------------------------------------------------------------------ A: weight gradient, bounds
def _wg_ref(shape, kind, ksize, cout):
    def make():
        x, dy = H.wgrad_case(shape, kind, cout)
        dw, mag, terms = H.wgrad_reference(x, dy, ksize)
        return x, dy, dw, H.bound_wgrad(mag, terms)
    return cached(("wg", shape, kind, ksize, cout), make)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", H.WGRAD_SMALL)
def test_wgrad3x3_within_bound_both_forms(ops, monkeypatch, shape, kind):
    x, dy, ref, bound = _wg_ref(shape, kind, 3, 128)
    assert shape[0] * shape[1] * shape[2] <= 4000
    xd, dd = nchw(x, KINDS[kind]), nchw(dy, KINDS[kind])
    got = {}
    for form in ("tap", "row"):
        set_form(monkeypatch, form)
        dw = ops.conv2d_wgrad(xd, dd)
        assert dw.shape == (128, 128, 3, 3) and dw.dtype == torch.float32
        assert torch.equal(dw, ops.conv2d_wgrad(xd, dd)), "not run-to-run identical"
        r = H.worst(dw.cpu().numpy(), ref, bound)
        print(f"wgrad3x3 {form} {shape} {kind}: error / bound {r:.4f}")
        note(("wgrad3x3", form if shape[2] >= 16 else "tap", kind), r)
        assert r <= 1.0, (form, r)
        got[form] = dw
    if shape[2] < 16:                                            # NARROW: the row request falls back to the tap form
        assert torch.equal(got["tap"], got["row"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cout", [128, 64])
@pytest.mark.parametrize("shape", H.WGRAD_ONE_TAP)
def test_wgrad_one_tap_within_bound(ops, shape, cout, kind):
    """k = 1: the deblock (cout 128) and the stacked heads (cout 64: dy is a genuine 64-channel channels-last tensor, the dyc form)."""
    x, dy, ref, bound = _wg_ref(shape, kind, 1, cout)
    xd, dd = nchw(x, KINDS[kind]), nchw(dy, KINDS[kind])
    assert dd.shape[1] == cout and dd.is_contiguous(memory_format=torch.channels_last)
    dw = ops.conv2d_wgrad(xd, dd, 1)
    assert dw.shape == (cout, 128, 1, 1) and torch.equal(dw, ops.conv2d_wgrad(xd, dd, 1))
    r = H.worst(dw.cpu().numpy(), ref, bound)
    print(f"wgrad1x1 cout {cout} {shape} {kind}: error / bound {r:.4f}")
    note(("wgrad1x1", cout, kind), r)
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------ B: weight gradient, integers
def _int_case(shape, ksize=3, cout=128):
    def make():
        x, dy = H.integer_case(shape, cout)
        return torch.from_numpy(x), torch.from_numpy(dy), H.integer_reference(x, dy, ksize)
    return cached(("int", shape, ksize, cout), make)


def _int_run(ops, shape, kind, ksize=3, cout=128):
    x8, d8, ref = _int_case(shape, ksize, cout)
    xd = x8.cuda().to(KINDS[kind]).permute(0, 3, 1, 2)
    dd = d8.cuda().to(KINDS[kind]).permute(0, 3, 1, 2)
    return lambda: ops.conv2d_wgrad(xd, dd, ksize).cpu().numpy(), ref


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", H.WGRAD_SMALL)
def test_wgrad3x3_integers_exact_small(ops, monkeypatch, shape, kind):
    """A single lost or doubled pixel changes an integer: every small shape, both forms."""
    run, ref = _int_run(ops, shape, kind)
    for form in ("tap", "row"):
        set_form(monkeypatch, form)
        got = run()
        assert np.array_equal(got, ref), (form, int((got != ref).sum()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [H.WGRAD_INT_TAP_LAST, H.WGRAD_INT_ROW_FIRST])
def test_wgrad3x3_integers_exact_across_the_row_threshold(ops, monkeypatch, shape, kind):
    """SEC_WGRAD_ROW unset: 159 999 pixels take the tap form, 160 000 the row form (wgrad_plan restates the host's decision; the weight
    gradient does not report through last_kernel_name, so the automatic run is held to the integer reference like both forced runs:
    all three are bit-equal)."""
    pixels = shape[0] * shape[1] * shape[2]
    assert H.wgrad_plan(pixels, shape[2], 9, None)[0] == ("row" if pixels >= 160000 else "tap")
    run, ref = _int_run(ops, shape, kind)
    for form in (None, "tap", "row"):
        set_form(monkeypatch, form)
        got = run()
        assert np.array_equal(got, ref), (form, int((got != ref).sum()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [H.WGRAD_INT_RESLICE, H.WGRAD_INT_TRAIN])
def test_wgrad3x3_integers_exact_large(ops, monkeypatch, shape, kind):
    """692 224 pixels: above the 688 128 from which the tap form has more than 256 slices and re-slices; 4 x 200 x 176: car.fhd."""
    pixels = shape[0] * shape[1] * shape[2]
    if shape == H.WGRAD_INT_RESLICE:
        assert pixels > H.WGRAD_RESLICE_ABOVE and H.wgrad_plan(pixels, shape[2], 9, False)[1] != 42
    run, ref = _int_run(ops, shape, kind)
    for form in ("tap", "row"):
        set_form(monkeypatch, form)
        got = run()
        assert np.array_equal(got, ref), (form, int((got != ref).sum()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cout", [64, 128])
def test_wgrad_one_tap_integers_exact_at_the_training_shape(ops, cout, kind):
    run, ref = _int_run(ops, H.WGRAD_INT_TRAIN, kind, 1, cout)
    got = run()
    assert got.shape == (cout, 128, 1, 1) and np.array_equal(got, ref), int((got != ref).sum())


# ------------------------------------------------------------------------------------------------ C: the autograd functions
def _function_inputs(kind, cout, seed):
    b, h, w = H.FUNCTION_SHAPE
    rng = np.random.default_rng(seed)
    x = H.round16(rng.standard_normal((b, h, w, 128), np.float32), kind)
    dy = H.round16(rng.standard_normal((b, h, w, cout), np.float32) / 8, kind)
    return x, dy, rng


def _check(name, kind, got, ref, bound):
    r = H.worst(got, ref, bound)
    print(f"{name} {kind}: error / bound {r:.4f}")
    note((name, kind), r)
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("kind", KINDS)
def test_conv3x3_function_fp64(ops, kind):
    x, dy, rng = _function_inputs(kind, 128, 3)
    w = (rng.standard_normal((128, 128, 3, 3)) / 34).astype(np.float32)      # plain random: asymmetric in the taps and in (co, ci)
    w16 = H.round16(w, kind)
    xd = nchw(x, KINDS[kind]).requires_grad_()
    wd = torch.from_numpy(w).cuda().requires_grad_()
    y = ops.Conv3x3Function.apply(xd, wd)
    y.backward(nchw(dy, KINDS[kind]))
    assert y.dtype == KINDS[kind] and xd.grad.dtype == KINDS[kind] and wd.grad.dtype == torch.float32
    ref, mag, t = H.conv_reference(x, w16)
    _check("Conv3x3.y", kind, nhwc_np(y), ref, H.bound_conv(ref, mag, t, kind))
    ref, mag, t = H.conv_reference(dy, w16, transposed_dgrad=True)
    _check("Conv3x3.dx", kind, nhwc_np(xd.grad), ref, H.bound_conv(ref, mag, t, kind))
    ref, mag, terms = H.wgrad_reference(x, dy, 3)
    _check("Conv3x3.dW", kind, wd.grad.cpu().numpy(), ref, H.bound_wgrad(mag, terms))


@pytest.mark.parametrize("kind", KINDS)
def test_conv_transpose_1x1_function_fp64(ops, kind):
    """weight [Cin, Cout, 1, 1]: y[co] = sum_ci x[ci] W[ci][co] is the 1x1 convolution with W^T, dx the 1x1 convolution with W."""
    x, dy, rng = _function_inputs(kind, 128, 4)
    w = (rng.standard_normal((128, 128, 1, 1)) / 11).astype(np.float32)
    w16 = H.round16(w, kind)
    xd = nchw(x, KINDS[kind]).requires_grad_()
    wd = torch.from_numpy(w).cuda().requires_grad_()
    y = ops.ConvTranspose1x1Function.apply(xd, wd)
    y.backward(nchw(dy, KINDS[kind]))
    ref, mag, t = H.conv_reference(x, np.ascontiguousarray(w16.transpose(1, 0, 2, 3)))
    _check("ConvT1x1.y", kind, nhwc_np(y), ref, H.bound_conv(ref, mag, t, kind))
    ref, mag, t = H.conv_reference(dy, w16)
    _check("ConvT1x1.dx", kind, nhwc_np(xd.grad), ref, H.bound_conv(ref, mag, t, kind))
    ref, mag, terms = H.wgrad_reference(x, dy, 1)                 # [co][ci]; the transposed conv's weight is [ci][co]
    assert wd.grad.dtype == torch.float32 and wd.grad.shape == wd.shape
    _check("ConvT1x1.dW", kind, wd.grad.cpu().numpy(), ref.transpose(1, 0, 2, 3), H.bound_wgrad(mag, terms).transpose(1, 0, 2, 3))


@pytest.mark.parametrize("kind", KINDS)
def test_heads_1x1_function_fp64(ops, kind):
    x, dy, rng = _function_inputs(kind, 64, 5)
    w = (rng.standard_normal((64, 128, 1, 1)) / 11).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32)
    w16 = H.round16(w, kind)
    xd = nchw(x, KINDS[kind]).requires_grad_()
    wd, bd = torch.from_numpy(w).cuda().requires_grad_(), torch.from_numpy(bias).cuda().requires_grad_()
    y = ops.Heads1x1Function.apply(xd, wd, bd)
    y.backward(nchw(dy, KINDS[kind]))
    ref, mag, t = H.conv_reference(x, w16, bias=bias)
    _check("Heads.y", kind, nhwc_np(y), ref, H.bound_conv(ref, mag, t, kind, bias=True))
    ref, mag, t = H.conv_reference(dy, w16, transposed_dgrad=True)
    assert t == 64
    _check("Heads.dx", kind, nhwc_np(xd.grad), ref, H.bound_conv(ref, mag, t, kind))
    ref, mag, terms = H.wgrad_reference(x, dy, 1)
    _check("Heads.dW", kind, wd.grad.cpu().numpy(), ref, H.bound_wgrad(mag, terms))
    d64 = dy.astype(np.float64).reshape(-1, 64)
    _check("Heads.db", kind, bd.grad.cpu().numpy(), d64.sum(0), H.bound_sum32(np.abs(d64).sum(0), len(d64)))


# ------------------------------------------------------------------------------------------------ D: the one-launch weight pack
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cout,cin,k", H.PACK_SHAPES)
def test_pack_weight_train_equals_the_separate_packs(ops, cout, cin, k, kind):
    from second_amd import runtime as rt
    dt = KINDS[kind]
    w = torch.from_numpy(np.random.default_rng(cout + cin + k).standard_normal((cout, cin, k, k)).astype(np.float32)).cuda()
    ref_f = ops.conv2d_pack_weight(w.to(dt))
    ref_d = ops.conv2d_pack_weight(ops.conv2d_dgrad_weight(w.to(dt)))
    assert ref_f is not None and ref_d is not None
    total = k * k * cin * cout
    assert ref_f.numel() == total + 8 and float(ref_f[total:].float().abs().max()) == 0.0     # the 16-byte zero block
    pk_f, pk_d = ops.conv2d_pack_weight_train(w, dt)
    assert torch.equal(pk_f, ref_f) and torch.equal(pk_d, ref_d)
    # the same launch into buffers full of ones with a guard behind them: the zero block is WRITTEN, nothing behind it is
    buf = torch.ones((2, total + 16), dtype=dt, device="cuda")
    l = rt.lib()
    rt.check(l.sec_conv2d_pack_weight_train(rt.ptr(w), cout, cin, k, rt.dtype_code(dt), rt.ptr(buf[0]), rt.ptr(buf[1]), rt.stream()),
             "sec_conv2d_pack_weight_train")
    for i, ref in ((0, ref_f), (1, ref_d)):
        assert torch.equal(buf[i, :total + 8], ref) and float(buf[i, total + 8:].float().min()) == 1.0


# ------------------------------------------------------------------------------------------------ E: BatchNorm + ReLU
def _bn_run(ops, case, kind, relu, live=None, sentinel=None):
    """Forward (running statistics from the case's non-trivial values) and backward on [P, C] rows.  live: through rows_dev.  sentinel:
    z and dy are pre-filled buffers handed to the C entry points (the wrappers allocate their own), to see what is NOT written."""
    from second_amd import runtime as rt
    dt = KINDS[kind]
    y = torch.from_numpy(case["y"]).cuda().to(dt)
    dz = torch.from_numpy(case["dz"]).cuda().to(dt)
    ga, be = torch.from_numpy(case["gamma"]).cuda(), torch.from_numpy(case["beta"]).cuda()
    rm, rv = torch.from_numpy(case["running_mean"]).cuda(), torch.from_numpy(case["running_var"]).cuda()
    rows = None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")
    if sentinel is None:
        z, mean, invstd = ops.bn_relu_forward(y, ga, be, H.BN_EPS, H.BN_MOMENTUM, rm, rv, relu, rows_dev=rows)
        z2 = ops.bn_relu_forward(y, ga, be, H.BN_EPS, H.BN_MOMENTUM, None, None, relu, rows_dev=rows)[0]
        n = y.shape[0] if live is None else min(max(live, 0), y.shape[0])
        assert torch.equal(z[:n], z2[:n]), "z depends on the running statistics being given"
        dy, dgamma, dbeta = ops.bn_relu_backward(dz, y, ga, be, mean, invstd, relu, rows_dev=rows)
    else:
        p, c = y.shape
        l = rt.lib()
        ws = rt.workspace(l.sec_bn_train_workspace_bytes(c), y.device)
        z, dy = torch.full_like(y, sentinel), torch.full_like(y, sentinel)
        mean, invstd, dgamma, dbeta = (torch.full((c,), float("nan"), device="cuda") for _ in range(4))
        rt.check(l.sec_bn_relu_fwd_nhwc(rt.ptr(y), p, c, rt.ptr(ga), rt.ptr(be), float(H.BN_EPS), float(H.BN_MOMENTUM), rt.ptr(rm), rt.ptr(rv),
                                        int(relu), rt.ptr(z), rt.ptr(mean), rt.ptr(invstd), rt.ptr(ws), ws.numel(), rt.dtype_code(dt),
                                        rt.ptr(rows), rt.stream()), "sec_bn_relu_fwd_nhwc")
        rt.check(l.sec_bn_relu_bwd_nhwc(rt.ptr(dz), rt.ptr(y), p, c, rt.ptr(ga), rt.ptr(be), rt.ptr(mean), rt.ptr(invstd), int(relu),
                                        rt.ptr(dy), rt.ptr(dgamma), rt.ptr(dbeta), rt.ptr(ws), ws.numel(), rt.dtype_code(dt), rt.ptr(rows),
                                        rt.stream()), "sec_bn_relu_bwd_nhwc")
    f = lambda t: t.float().cpu().numpy()
    return dict(z=f(z), dy=f(dy), mean=f(mean), invstd=f(invstd), running_mean=f(rm), running_var=f(rv), dgamma=f(dgamma), dbeta=f(dbeta))


def _bn_hold(case, kind, relu, got, tag, live=None):
    ref = H.BnRef(case["y"], case["dz"], case["gamma"], case["beta"], H.BN_EPS, H.BN_MOMENTUM, relu, live, case["running_mean"],
                  case["running_var"], kind)
    assert ref.ambiguous_fraction <= H.AMBIGUOUS_CAP
    r = ref.channel_ratios(got["mean"], got["invstd"], got["running_mean"], got["running_var"], got["dbeta"], got["dgamma"])
    r.update(ref.worst_elements(got["z"], got["dy"]))
    print(f"bn {tag} {case['y'].shape} {kind} relu {relu} live {live}: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    for name, v in r.items():
        note(("bn " + tag, name, kind), v)
        assert v <= 1.0, (name, v)
    return ref


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("c", H.BN_CHANNELS)
def test_bn_small_path_fp64(ops, c, relu, kind):
    """k_bn_partial over 128 groups + k_bn_apply_small: 1, 2, 255 and 2 325 rows (one row: variance 0, invstd 1 / sqrt(eps), the
    kernel's biased-variance rule for the running update)."""
    for p in H.BN_SMALL_P:
        case = H.bn_case(p, c, kind)
        _bn_hold(case, kind, relu, _bn_run(ops, case, kind, relu), "small")


@pytest.mark.parametrize("kind", KINDS)
def test_bn_channels_last_image_equals_its_rows(ops, kind):
    """The [B, C, H, W] channels_last form (BatchNorm2d of the RPN) is the same memory as [B H W, C] rows: same bits."""
    dt = KINDS[kind]
    case = H.bn_case(2325, 128, kind)
    y = torch.from_numpy(case["y"]).cuda().to(dt)
    ga, be = torch.from_numpy(case["gamma"]).cuda(), torch.from_numpy(case["beta"]).cuda()
    y4 = y.view(3, 25, 31, 128).permute(0, 3, 1, 2)
    z2, m2, i2 = ops.bn_relu_forward(y, ga, be, H.BN_EPS, H.BN_MOMENTUM, None, None, True)
    z4, m4, i4 = ops.bn_relu_forward(y4, ga, be, H.BN_EPS, H.BN_MOMENTUM, None, None, True)
    assert torch.equal(z4.permute(0, 2, 3, 1).reshape(2325, 128), z2) and torch.equal(m2, m4) and torch.equal(i2, i4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("c", H.BN_SWITCH_C)
@pytest.mark.parametrize("p", H.BN_SWITCH_P)
def test_bn_across_the_path_switch_fp64(ops, p, c, relu, kind):
    """131 072 rows: the last size of the two-launch path; 131 073: the first of k_bn_partial over 512 groups + k_bn_*_finalize +
    k_bn_apply (the path car.fhd's RPN takes at batch 4), the smallest size at which it exists."""
    assert H.bn_chain(p, p, c)[0] == (128 if p <= H.BN_SMALL_ROWS else 512)
    case = H.bn_case(p, c, kind)
    _bn_hold(case, kind, relu, _bn_run(ops, case, kind, relu), "small" if p <= H.BN_SMALL_ROWS else "large")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("p", H.BN_OFFSET_P)
def test_bn_offset_mean_fp64(ops, p, relu, kind):
    """Channels whose mean is 8 x (fp16) / 4 x (bf16) their standard deviation: E[y^2] - E[y]^2 loses four to six bits to
    cancellation, which the double combine must absorb; a constant channel (variance exactly 0) and an all-zero channel."""
    case = H.bn_case(p, H.BN_OFFSET_C, kind, "offset")
    ref = _bn_hold(case, kind, relu, _bn_run(ops, case, kind, relu), "offset")
    assert ref.var[1] == 0.0 and ref.var[2] == 0.0 and ref.mean[2] == 0.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", H.BN_CAP_P)
def test_bn_static_capacity_fp64(ops, p, kind):
    """rows_dev on a buffer of P rows, live in {0, 1, 1 000, P, P + 5}: NaN in y and dz behind the live rows, a sentinel in z and dy.
    The live rows meet the bounds of a tensor of exactly `live` rows (summed by the path the CAPACITY selects); rows behind them are
    untouched; nothing is NaN.  live = 0 / 1 follow the kernel's documented rule (BnRef), not torch's."""
    c = H.BN_CAP_C
    base = H.bn_case(p, c, kind)
    for live in H.bn_cap_lives(p):
        n = min(live, p)
        case = dict(base)
        case["y"], case["dz"] = base["y"].copy(), base["dz"].copy()
        case["y"][n:] = np.nan
        case["dz"][n:] = np.nan
        got = _bn_run(ops, case, kind, True, live=live, sentinel=-7.0)
        assert (got["z"][n:] == -7.0).all() and (got["dy"][n:] == -7.0).all(), "rows behind the live ones were written"
        for name, v in got.items():
            assert np.isfinite(v[:n] if name in ("z", "dy") else v).all(), (name, live)
        _bn_hold(case, kind, True, got, "capacity", live=live)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", H.BN_ROWS_C)
def test_batch_norm_relu_function_on_rows_fp64(ops, c, kind):
    """BatchNormReluFunction on the [N, C] feature rows of a sparse tensor (BatchNorm1d of the sparse stack) under autograd."""
    dt = KINDS[kind]
    case = H.bn_case(H.BN_ROWS_N, c, kind)
    y = torch.from_numpy(case["y"]).cuda().to(dt).requires_grad_()
    ga, be = torch.from_numpy(case["gamma"]).cuda().requires_grad_(), torch.from_numpy(case["beta"]).cuda().requires_grad_()
    rm, rv = torch.from_numpy(case["running_mean"]).cuda(), torch.from_numpy(case["running_var"]).cuda()
    z = ops.BatchNormReluFunction.apply(y, ga, be, rm, rv, H.BN_EPS, H.BN_MOMENTUM, True)
    z.backward(torch.from_numpy(case["dz"]).cuda().to(dt))
    f = lambda t: t.detach().float().cpu().numpy()
    got = dict(z=f(z), dy=f(y.grad), mean=None, invstd=None, running_mean=f(rm), running_var=f(rv), dgamma=f(ga.grad), dbeta=f(be.grad))
    _bn_hold(case, kind, True, got, "rows")


def test_report_ratios():
    for k in sorted(RATIOS, key=str):
        print("device", k, f"{RATIOS[k]:.4f}")
