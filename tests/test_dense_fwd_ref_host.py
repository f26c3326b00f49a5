"""CPU: the float64 reference, the per-element bound and the exact-integer cases of tests/dense_fwd_ref_helpers.py before the GPU tests
rely on them, and the host-only refusals of conv2d_fwd_decide.

1. conv2d_reference == torch.nn.functional.conv2d in double for every (k, stride, pad) of the case table: odd maps under stride 2 and
   k = stride (last tap row / column in the padding or dropped), a 1 x 1 map; conv2d_terms == the convolution of ones.
2. The bound holds for the reference rounded to the 16-bit type on every case of the table, and for a plain fp32 accumulation in two
   orders on its small cases (the threshold maps and the long thin ones get the reference-alone check only: 2 - 5 s each).
3. Seven seeded faults on a numpy model of the launch (fp32 accumulation, bias, ReLU, one rounding).  Each must be REJECTED by the
   new checks -- bit equality on integer data, the per-element bound on Gaussian data -- and the two existing checks are asked too
   (test_report_mutations prints the list).  What they answer, bf16 / fp16 alike:
     corner tap          new: rejected   old: both reject -- a whole tap of 128 products moves the 256 channels of that pixel by ~0.3
                         sigma, far over either old limit (the old checks do see this one, on every case tried)
     bias block          new: rejected   old: the per-element check ACCEPTS (its launch has no bias); the maximum check rejects
     ReLU before bias    new: rejected   old: the per-element check ACCEPTS (its launch has no ReLU); the maximum check rejects
     frame offset        new: rejected   old: both reject
     truncating store    new: rejected   old: the maximum check ACCEPTS everywhere (2^-7 / 2^-9 of the maximum is its limit); the
                         per-element check rejects on bf16 Gaussian data and ACCEPTS on fp16 Gaussian data (the accumulation
                         term it grants twice is larger than an fp16 ulp) and on bf16 integers
     unwritten tile      new: rejected   old: both reject
     into overwrite      new: rejected   old: both ACCEPT (neither looks outside the written channel range)
   So for a fault of the epilogue the tensor-maximum check was the only guard, and for a store or an overwrite there was none.
   The printed list is the record; the assertions are on the new checks only.  The propagated bound of the two-stage kernels is
   loose (test_propagated_bound_...: the honest chain reaches 0.03 of it, one dropped mid channel stays inside): those kernels are
   pinned by their exact-integer cases.
4. The byte limits of conv2d_fwd_decide through ops.conv2d_plan_name, no allocation and no launch: both sides of each."""
import numpy as np
import pytest
import torch

import dense_fwd_ref_helpers as H

REPORT = {}


# ------------------------------------------------------------------------------------------------ 1: the reference is the convolution
GEOMETRIES = sorted({(c[3], c[4], c[5]) for c in H.FORM_CASES})
SMALL_MAPS = [(2, 1, 1), (1, 5, 7), (2, 6, 4), (1, 9, 8), (2, 4, 4)]


def _torch_conv(x, w, bias, k, s, p):
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float64)).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(xt, torch.from_numpy(np.asarray(w, np.float64)), None if bias is None else torch.from_numpy(np.asarray(bias, np.float64)), s, p)
    return y.permute(0, 2, 3, 1).numpy()


def test_geometries_are_the_ones_of_the_kernels():
    assert GEOMETRIES == [(1, 1, 0), (2, 2, 0), (3, 1, 1), (3, 2, 1), (4, 4, 0)]


@pytest.mark.parametrize("shape", SMALL_MAPS)
@pytest.mark.parametrize("k,s,p", GEOMETRIES)
def test_reference_is_torch_double(k, s, p, shape):
    b, h, w = shape
    if H.out_size(h, k, s, p) < 1 or H.out_size(w, k, s, p) < 1:
        h, w = h + k, w + k                                                       # (the 1 x 1 map under k = stride: k + 1, odd or even)
    rng = np.random.default_rng(k * 100 + s * 10 + h)
    x = rng.standard_normal((b, h, w, 12))
    wt = rng.standard_normal((5, 12, k, k))
    bias = rng.standard_normal(5)
    ref, mag, terms = H.conv2d_reference(x, wt, bias, k, s, p)
    want = _torch_conv(x, wt, bias, k, s, p)
    assert ref.shape == want.shape
    assert np.abs(ref - want).max() <= 1e-13 * np.abs(want).max()
    assert np.abs(mag - _torch_conv(np.abs(x), np.abs(wt), np.abs(bias), k, s, p)).max() <= 1e-13 * mag.max()
    ones = _torch_conv(np.ones((1, h, w, 12)), np.ones((1, 12, k, k)), None, k, s, p)[0, :, :, 0]
    assert np.array_equal(terms, ones.astype(np.int64))
    if p > 0:
        assert terms[0, 0] < 12 * k * k                                           # the corner counts only the taps inside the image
    # the float32 mode on integers is the same convolution, exactly
    xi, wi = rng.integers(-4, 5, x.shape), rng.integers(-2, 3, wt.shape)
    r32, none, _ = H.conv2d_reference(xi, wi, None, k, s, p, dtype=np.float32, want_mag=False)
    assert none is None and r32.dtype == np.float32 and np.array_equal(r32, _torch_conv(xi, wi, None, k, s, p))


def test_odd_maps_under_stride_two_drop_or_pad_the_last_tap():
    """3x3 / s2 / p1 on 5 x 7: the last output row reads rows 3, 4 and the padding row 5; on 6 x 4 the last window starts at row 3 and ends
    in the padding too, while 2x2 / s2 on 5 x 7 DROPS row 4 and column 6."""
    x = np.arange(35, dtype=np.float64).reshape(1, 5, 7, 1) + 1
    ref, _, terms = H.conv2d_reference(x, np.ones((1, 1, 3, 3)), None, 3, 2, 1)
    assert ref.shape == (1, 3, 4, 1) and terms[2, 3] == 4 and ref[0, 2, 3, 0] == x[0, 3:5, 5:7, 0].sum()
    ref, _, terms = H.conv2d_reference(x, np.ones((1, 1, 2, 2)), None, 2, 2, 0)
    assert ref.shape == (1, 2, 3, 1) and (terms == 4).all() and ref.sum() == x[0, :4, :6, 0].sum()


# ------------------------------------------------------------------------------------------------ 2: the bound holds for honest arithmetic
GAUSS = [c for c in H.FORM_CASES if c[8] and c[6][1] * c[6][2] <= 1200]


def _fp32_orders(x, wt, bias, k, s, p):
    """Two plain fp32 accumulations of the same products: taps forward over whole channel rows; taps backward, the channels in four
    strided groups added one after the other."""
    b, h, w, cin = x.shape
    ho, wo = H.out_size(h, k, s, p), H.out_size(w, k, s, p)
    xp = H._ringed(np.asarray(x, np.float32), p)
    w32 = np.asarray(wt, np.float32)
    taps = [(ky, kx) for ky in range(k) for kx in range(k)]
    a = np.zeros((b * ho * wo, w32.shape[0]), np.float32)
    for ky, kx in taps:
        a = a + H._tap(xp, ky, kx, s, ho, wo) @ w32[:, :, ky, kx].T
    c = np.zeros_like(a)
    for ky, kx in taps[::-1]:
        t = H._tap(xp, ky, kx, s, ho, wo)
        for g in range(4):
            c = c + t[:, g::4] @ w32[:, g::4, ky, kx].T
    shape = (b, ho, wo, w32.shape[0])
    return [(v + np.asarray(bias, np.float32)).reshape(shape) for v in (a, c)]


@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("case", GAUSS, ids=H.case_id)
def test_bound_holds_for_the_reference_alone_and_for_fp32_in_two_orders(case, kind):
    form, cin, cout, k, s, p, shape, name, _ = case
    x, wt, bias = H.gaussian_case(cin, cout, k, shape, kind)
    ref, mag, terms = H.conv2d_reference(x, wt, bias, k, s, p)
    bound = H.bound_fwd(ref, mag, terms, kind, True)
    r = H.worst(H.round16(ref, kind), ref, bound)
    REPORT[("reference alone", kind)] = max(REPORT.get(("reference alone", kind), 0.0), r)
    assert r <= 1.0, r
    for i, acc in enumerate(_fp32_orders(x, wt, bias, k, s, p)):
        for relu in (False, True):
            y = H.round16(np.maximum(acc, 0) if relu else acc, kind)
            r = H.worst(y, np.maximum(ref, 0) if relu else ref, bound)
            REPORT[("fp32 order %d" % i, kind)] = max(REPORT.get(("fp32 order %d" % i, kind), 0.0), r)
            assert r <= 1.0, (i, relu, r)


LARGE = [c for c in H.FORM_CASES if c not in GAUSS]


@pytest.mark.parametrize("case", LARGE, ids=H.case_id)
def test_bound_holds_for_the_reference_alone_on_the_large_cases(case):
    """The rest of the table (the threshold maps and the long thin ones): one float64 reference per case on bf16-rounded operands, its
    rounding to either output type inside that type's bound."""
    form, cin, cout, k, s, p, shape, name, _ = case
    x, wt, bias = H.gaussian_case(cin, cout, k, shape, "bf16")
    ref, mag, terms = H.conv2d_reference(x, wt, bias, k, s, p)
    for kind in H.KINDS:
        r = H.worst(H.round16(ref, kind), ref, H.bound_fwd(ref, mag, terms, kind, True))
        REPORT[("reference alone", kind)] = max(REPORT.get(("reference alone", kind), 0.0), r)
        assert r <= 1.0, (kind, r)


@pytest.mark.parametrize("kind", H.KINDS)
def test_propagated_bound_holds_for_a_rounded_three_stage_chain(kind):
    """conv -> 16 bit -> 1x1 -> 16 bit -> 1x1 -> 16 bit in fp32 (the tail's roundings): inside the propagated bound; the same chain
    with the second intermediate kept in fp32 too (fewer roundings); and NOT inside it when the inner ReLU is skipped."""
    x, wt, bias = H.gaussian_case(128, 128, 3, (2, 9, 17), kind)
    rng = np.random.default_rng(5)
    w1 = H.round16(rng.standard_normal((128, 128), np.float32) / np.float32(128 ** 0.5), kind)
    w2 = H.round16(rng.standard_normal((64, 128), np.float32) / np.float32(128 ** 0.5), kind)
    b1, b2 = rng.standard_normal(128).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    ref0, mag0, terms = H.conv2d_reference(x, wt, bias, 3, 1, 1)
    bd0 = H.bound_fwd(ref0, mag0, terms, kind, True)
    ref2, bd2 = H.chain_reference(None, w1, b1, True, w2, b2, kind, x_ref=np.maximum(ref0, 0), x_bound=bd0)
    y0 = H.round16(np.maximum(_fp32_orders(x, wt, bias, 3, 1, 1)[0], 0), kind)
    for keep_mid in (False, True):
        mid = np.maximum(y0.reshape(-1, 128) @ w1.T + b1, 0).astype(np.float32)
        mid = mid if keep_mid else H.round16(mid, kind)
        y = H.round16((mid @ w2.T + b2).astype(np.float32), kind).reshape(ref2.shape)
        r = H.worst(y, ref2, bd2)
        REPORT[("three-stage chain", kind)] = max(REPORT.get(("three-stage chain", kind), 0.0), r)
        assert r <= 1.0, r
    # What a worst-case propagation costs: every stage multiplies the carried bound by sum |w| of a row (~9 for 128 N(0, 1/128)
    # weights) where the errors really add like sqrt(128) -- the honest chain sits at a few percent of the bound, and a fault has to
    # be gross to leave it: a skipped inner ReLU does, one dropped mid channel does NOT.  The exact-integer tail and chain cases of
    # the GPU module are what pins those two kernels per product.
    mid = H.round16((y0.reshape(-1, 128) @ w1.T + b1).astype(np.float32), kind)
    assert H.worst(H.round16((mid @ w2.T + b2).astype(np.float32), kind).reshape(ref2.shape), ref2, bd2) > 1.0
    mid = H.round16(np.maximum(y0.reshape(-1, 128) @ w1.T + b1, 0).astype(np.float32), kind)
    mid[:, 77] = 0
    r = H.worst(H.round16((mid @ w2.T + b2).astype(np.float32), kind).reshape(ref2.shape), ref2, bd2)
    REPORT[("three-stage chain, one mid channel dropped (NOT caught by the bound)", kind)] = r


# ------------------------------------------------------------------------------------------------ 3: mutations
MUTATIONS = ["corner tap", "bias block", "relu before bias", "frame offset", "truncating store", "unwritten tile", "into overwrite"]
M_CIN, M_COUT, M_SHAPE = 128, 256, (2, 9, 17)            # two channel blocks of 128, four 8 x 16 tiles per frame, ragged bottom and right
SENTINEL = -77.0


def _truncate16(a, kind):
    """fp32 -> the 16-bit type by dropping the low mantissa bits (towards zero), as float32."""
    if kind == "bf16":
        return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r = a.astype(np.float16)
    over = np.abs(r.astype(np.float32)) > np.abs(a)
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float32)


def model_launch(x, wt, bias, relu, kind, mut=None, wide=0, offset=0):
    """What a launch writes, [B,H,W,cout] float32 of 16-bit values (3x3 / s1 / p1): fp32 accumulation, + bias, ReLU, one rounding --
    with one seeded fault.  wide > 0: the `into` form, the result inside a sentinel-filled [B,H,W,wide] tensor at `offset`."""
    b, h, w, cin = x.shape
    cout = wt.shape[0]
    acc, _, _ = H.conv2d_reference(x, wt, None, 3, 1, 1, dtype=np.float32, want_mag=False)
    if mut == "corner tap":                                     # tap (0, 0) of the ragged corner pixel of frame 0 never arrives
        acc[0, h - 1, w - 1] -= np.asarray(wt[:, :, 0, 0], np.float32) @ np.asarray(x[0, h - 2, w - 2], np.float32)
    if mut == "frame offset":                                   # tile 1 of frame 1 computed from frame 0's pixels
        acc[1, 0:8, 16:32] = acc[0, 0:8, 16:32]
    bv = np.zeros(cout, np.float32) if bias is None else np.asarray(bias, np.float32).copy()
    if mut == "bias block":
        bv[128:256] = bv[0:128]
    if mut == "relu before bias" and relu:
        v = np.maximum(acc, 0) + bv
    else:
        v = acc + bv
        v = np.maximum(v, 0) if relu else v
    y = _truncate16(v, kind) if mut == "truncating store" else H.round16(v, kind)
    if mut == "unwritten tile":
        y[1, 8:16, 0:16] = 0.0                                  # what fresh memory usually holds
    if not wide:
        return y
    out = np.full((b, h, w, wide), SENTINEL, np.float32)
    out[..., offset:offset + cout] = y
    if mut == "into overwrite":
        out[..., offset + cout] = y[..., 0]
    return out


def _mutation_data(data, kind):
    if data == "integer":
        x, wt, bias, pre = H.integer_case(M_CIN, M_COUT, 3, M_SHAPE, 3)
        assert np.abs(pre).max() < 2 ** 24 and (pre == 0).mean() > 0 and (pre < 0).mean() > 0
        if kind == "bf16":
            assert (np.abs(pre) > 256).any()                    # values that bf16 has to round: the store matters
        return x.astype(np.float32), wt.astype(np.float32), bias.astype(np.float32)
    return H.gaussian_case(M_CIN, M_COUT, 3, M_SHAPE, kind, seed=1)


def new_check(data, kind, x, wt, bias, relu, y, wide=0, offset=0):
    """The check of tests/test_gpu_dense_fwd_fp64.py: bits on integers, the per-element bound on Gaussian data; for `into` every channel
    outside the written range keeps the sentinel's bits."""
    cout = wt.shape[0]
    if wide:
        outside = np.delete(y, np.s_[offset:offset + cout], axis=3)
        if not np.array_equal(H.bits_of(outside, kind), H.bits_of(np.full_like(outside, SENTINEL), kind)):
            return False
        y = y[..., offset:offset + cout]
    if data == "integer":
        pre, _, _ = H.conv2d_reference(x, wt, bias, 3, 1, 1, dtype=np.float32, want_mag=False)
        return bool(np.array_equal(H.bits_of(y, kind), H.rounded_bits(pre, relu, kind)))
    ref, mag, terms = H.conv2d_reference(x, wt, bias, 3, 1, 1)
    return H.worst(y, np.maximum(ref, 0) if relu else ref, H.bound_fwd(ref, mag, terms, kind, bias is not None)) <= 1.0


def old_checks(kind, x, wt, bias, mut, wide=0, offset=0):
    """The two existing checks on the launches THEY make: with bias and ReLU against the tensor maximum; without either per element
    (both against an fp32 reference, both on the channel slice only)."""
    cout = wt.shape[0]
    sl = np.s_[..., offset:offset + cout] if wide else np.s_[...]
    ref, _, _ = H.conv2d_reference(x, wt, bias, 3, 1, 1)
    a = H.old_check_max(model_launch(x, wt, bias, True, kind, mut, wide, offset)[sl], np.maximum(ref, 0), kind)
    ref0, mag0, _ = H.conv2d_reference(x, wt, None, 3, 1, 1)
    y0 = model_launch(x, wt, None, False, kind, mut, wide, offset)[sl]
    return a and H.old_check_max(y0, ref0, kind), H.old_check_per_element(y0, ref0, mag0, M_CIN, 3, kind)


@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("data", ["integer", "gaussian"])
def test_the_unmutated_model_passes_every_check(data, kind):
    x, wt, bias = _mutation_data(data, kind)
    for relu in (True, False):
        assert new_check(data, kind, x, wt, bias, relu, model_launch(x, wt, bias, relu, kind))
        assert new_check(data, kind, x, wt, bias, relu, model_launch(x, wt, bias, relu, kind, None, 384, 64), 384, 64)
    assert old_checks(kind, x, wt, bias, None) == (True, True)


@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("data", ["integer", "gaussian"])
@pytest.mark.parametrize("mut", MUTATIONS)
def test_mutation_is_rejected_by_the_new_check(mut, data, kind):
    x, wt, bias = _mutation_data(data, kind)
    wide, offset = (384, 64) if mut == "into overwrite" else (0, 0)
    if mut == "truncating store" and data == "integer" and kind == "fp16":
        # every integer below 2 048 IS an fp16 number: truncation and rounding agree on this data, there is nothing to reject
        assert np.abs(H.conv2d_reference(x, wt, bias, 3, 1, 1, dtype=np.float32, want_mag=False)[0]).max() < 2048
        REPORT[(mut, data, kind)] = "not a fault on this data (all values exact in fp16)"
        return
    verdicts = [new_check(data, kind, x, wt, bias, relu, model_launch(x, wt, bias, relu, kind, mut, wide, offset), wide, offset)
                for relu in (True, False)]
    old_max, old_elem = old_checks(kind, x, wt, bias, mut, wide, offset)
    REPORT[(mut, data, kind)] = "new check: rejected; old maximum check: %s; old per-element check (no bias, no ReLU): %s" % (
        "ACCEPTED" if old_max else "rejected", "ACCEPTED" if old_elem else "rejected")
    # a fault of the epilogue exists only in the launch that has one; every other fault in both
    assert not verdicts[0], "accepted with ReLU"
    if mut != "relu before bias":
        assert not verdicts[1], "accepted without ReLU"


def test_integer_cases_stay_exact_and_carry_the_relu_edge():
    for c in H.FORM_CASES:
        form, cin, cout, k, s, p, shape = c[:7]
        if shape[0] * shape[1] * shape[2] > 1200:
            continue                                            # (the large ones are built, and asserted inside integer_case, on the GPU run)
        x, wt, bias, pre = H.integer_case(cin, cout, k, shape, 0, s, p)
        assert np.abs(x).max() <= 4 and np.abs(wt).max() <= 2 and np.abs(bias).max() <= 8
        assert np.abs(pre).max() <= 8 * cin * k * k + 8 <= 18440 < 2 ** 24
        assert (pre == 0).mean() > 0 and (pre < 0).mean() > 0, H.case_id(c)
    w1, b1, w2, b2 = H.integer_chain_case(0)
    assert (np.abs(w1.reshape(128, 128)).sum(1) == 1).all() and (np.abs(w2.reshape(64, 128)).sum(1) == 4).all()


def test_case_table_names_every_instantiation():
    names = sorted({c[7] for c in H.FORM_CASES})
    assert names == sorted(H.INSTANTIATIONS)
    for n in H.INSTANTIATIONS:
        assert any(c[7] == n and c[8] for c in H.FORM_CASES), "no Gaussian case for " + n
    for what, on, past in H.THRESHOLDS:
        assert sum(c[:7] == on for c in H.FORM_CASES) == 1 and sum(c[:7] == past for c in H.FORM_CASES) == 1, what
    rounds = [(H.THRESHOLDS[0], 16, 16, 64), (H.THRESHOLDS[1], 4, 16, 128), (H.THRESHOLDS[2], 2, 16, 128), (H.THRESHOLDS[3], 8, 16, 64)]
    for (what, on, past), th, tw, per in rounds:
        assert H.workgroup_count(on, th, tw, per) == 1024 < H.workgroup_count(past, th, tw, per), what
    assert H.workgroup_count(H.THRESHOLDS[4][1], 8, 16, 64) == 2560 < H.workgroup_count(H.THRESHOLDS[4][2], 8, 16, 64) == 2562


def test_report_mutations():
    for key in sorted(REPORT, key=str):
        print(key, "->", REPORT[key] if isinstance(REPORT[key], str) else "largest error / bound %.3f" % REPORT[key])


# ------------------------------------------------------------------------------------------------ 4: host-only refusals
@pytest.fixture(scope="module")
def plan():
    from second_amd import ops

    def name(form, cin, cout, k, s, p, bhw, dtype=torch.bfloat16):
        return ops.conv2d_plan_name(bhw[0], bhw[1], bhw[2], cin, cout, k, s, p, dtype, form)
    return name


BF = "__hip_bfloat16"


def test_patch_forms_stop_at_two_gib_per_frame(plan):
    """hw * cin * 2 <= 0x7fffffff: 64 channels up to 4095 x 4097 = 2^24 - 1 pixels, 128 channels up to 47 x 178 481 = 2^23 - 1."""
    under, over = (1, 4095, 4097), (1, 4096, 4096)
    assert under[1] * under[2] * 64 * 2 <= 0x7fffffff < over[1] * over[2] * 64 * 2
    assert plan("plain", 64, 128, 3, 2, 1, under) == "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 1>" % BF
    assert plan("plain", 64, 128, 3, 2, 1, over) == "k_conv2d_nhwc_dma<%s, 128>" % BF
    assert plan("into", 64, 128, 3, 2, 1, under) == "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 1>" % BF
    assert plan("into", 64, 128, 3, 2, 1, over) == ""
    assert plan("plain", 64, 128, 4, 4, 0, under) == "k_conv2d_patch<%s, 64, 4, 4, 2, 16, 1>" % BF
    assert plan("plain", 64, 128, 4, 4, 0, over) == "k_conv2d_nhwc_dma<%s, 128>" % BF
    under, over = (1, 47, 178481), (1, 2048, 4096)
    assert under[1] * under[2] * 128 * 2 <= 0x7fffffff < over[1] * over[2] * 128 * 2
    assert plan("plain", 128, 128, 2, 2, 0, under) == "k_conv2d_patch<%s, 128, 2, 2, 4, 16, 1>" % BF
    assert plan("plain", 128, 128, 2, 2, 0, over) == "k_conv2d_nhwc_dma<%s, 128>" % BF
    assert plan("into", 128, 128, 2, 2, 0, under, torch.float16) == "k_conv2d_patch<__half, 128, 2, 2, 4, 16, 1>"
    assert plan("into", 128, 128, 2, 2, 0, over, torch.float16) == ""
    # 256 channels, 3x3 / s1: past the limit the layer is k_conv2d_halo_reg's (which it is anyway at that many workgroups)
    under, over = (1, 2047, 2049), (1, 2048, 2048)
    assert under[1] * under[2] * 256 * 2 <= 0x7fffffff < over[1] * over[2] * 256 * 2
    assert plan("plain", 256, 128, 3, 1, 1, over) == plan("plain", 256, 128, 3, 1, 1, under) == "k_conv2d_halo_reg<%s, 256, 4, 0, false>" % BF
    assert plan("plain", 256, 128, 1, 1, 0, under) == "k_conv2d_patch<%s, 256, 1, 1, 2, 16, 1>" % BF
    assert plan("plain", 256, 128, 1, 1, 0, over) == "k_conv2d_nhwc_dma<%s, 128>" % BF


def test_rows_form_stops_at_two_gib_of_site_map(plan):
    under, over = (1, 256999, 2089), (1, 16384, 32768)           # 2^29 - 1 and 2^29 cells of four bytes
    assert under[1] * under[2] * 4 <= 0x7fffffff < over[1] * over[2] * 4
    assert plan("rows", 64, 64, 3, 2, 1, under) == "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 2, true, true>" % BF
    assert plan("rows", 64, 128, 3, 2, 1, under) == "k_conv2d_patch<%s, 64, 3, 2, 8, 16, 1, true>" % BF
    assert plan("rows", 64, 64, 3, 2, 1, over) == "" and plan("rows", 64, 128, 3, 2, 1, over) == ""
    assert plan("rows", 64, 64, 3, 1, 1, (2, 23, 19)) == "" and plan("rows", 128, 128, 3, 2, 1, (2, 23, 19)) == ""


def test_x3_and_gather_forms_stop_at_two_gib_per_frame(plan):
    under, over = (1, 47, 178481), (1, 2048, 4096)               # hw * 256 < 2^31
    assert under[1] * under[2] * 256 < 2 ** 31 <= over[1] * over[2] * 256
    for form in ("x3", "x3_tiles"):
        assert plan(form, 128, 128, 3, 1, 1, under) == "k_conv2d_halo_reg<%s, 128, 8, 3, false, 1, true>" % BF
        assert plan(form, 128, 128, 3, 1, 1, over) == ""
        assert plan(form, 128, 128, 3, 1, 1, (2, 9, 17), torch.float16) == ""         # two bf16 planes: no fp16 form
    under, over = (1, 16383, 16385), (1, 16384, 16384)           # hw * 8 < 2^31
    assert under[1] * under[2] * 8 < 2 ** 31 <= over[1] * over[2] * 8
    assert plan("gather", 128, 128, 3, 1, 1, under) == "k_conv2d_halo_reg<%s, 128, 8, 3, true>" % BF
    assert plan("gather", 128, 128, 3, 1, 1, over) == ""
    # the list and tail forms have no such limit of their own, and exist for the 128-channel 3x3 layer only
    assert plan("tiles", 128, 256, 3, 1, 1, over) == "k_conv2d_halo_reg<%s, 128, 8, 3, false>" % BF
    assert plan("tail", 128, 256, 3, 1, 1, (2, 9, 17)) == "" and plan("tiles", 64, 128, 3, 1, 1, (2, 9, 17)) == ""


@pytest.mark.parametrize("form", ["plain", "into", "rows", "tiles", "tail", "x3", "x3_tiles", "gather"])
def test_fp32_and_odd_channel_counts_are_refused(plan, form):
    geo = (3, 2, 1) if form in ("into", "rows") else (3, 1, 1)
    cin = 64 if form in ("into", "rows") else 128
    assert plan(form, cin, 128, *geo, (2, 24, 20), torch.float32) == ""
    for bad_in, bad_out in ((cin + 32, 128), (cin, 96), (cin, 160)):
        assert plan(form, bad_in, bad_out, *geo, (2, 24, 20)) == "", (bad_in, bad_out)
