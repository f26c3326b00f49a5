"""CPU: the fp64 references and per-element bounds of tests/dense_train_ref_helpers.py before the GPU tests rely on them.  A numpy
float32 RESTATEMENT of each kernel's summation order (weight gradient: 64-pixel steps, slices, the four-chain reduce over slices; row
form: three shifted images with zeros at the row ends; BatchNorm: per-thread chains, the LDS pass, the double combine) stays within
the bounds on every case; twelve seeded wrong restatements do not -- against the bound on a small case and, for the weight gradient,
against bit equality on an integer case.  The thirteenth, a variance kept in float all the way, stays INSIDE the bound (0.92 of it):
test_fp32_variance_mutant_is_not_caught_and_why says why a worst-case bound cannot separate it.

What the max-relative tolerances of tests/test_gpu_train_dense.py do with the same mutants (test_old_tolerance_lets_mutants_through
prints the list): they let the float variance through and catch the others.  A single lost pixel at 4 x 200 x 176 moves the typical
element of dW by 2e-4 of the maximum, a tenth of the old limit of 2e-3; 0.3-0.5 % of the elements -- the products of that pixel's
largest channels, up to 4.7e-3 -- still cross it, so the old check sees such a fault with a margin of 2.4 at that size and, the
maximum growing with the square root of the pixel count, not at all from about 0.8 M pixels on; the integer cases see it at any size.

Every BatchNorm case keeps its ambiguous ReLU elements under 0.1 %."""
import numpy as np
import pytest

import dense_train_ref_helpers as H

KINDS = ["bf16", "fp16"]
RATIOS = {}                                                     # restatement -> largest error / bound reached (test_report_ratios)
OLD_PASSES = {}                                                 # mutant -> did the old tolerance let it through


def note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


# ------------------------------------------------------------------------------------------------ weight gradient restatement
def _reduce_slices(part):
    """k_conv2d_wgrad_reduce: four chains over groups of eight slices, the rest into chain 0, (s0 + s1) + (s2 + s3); float32."""
    groups = len(part)
    s = [np.zeros(part.shape[1:], np.float32) for _ in range(4)]
    g = 0
    while g + 8 <= groups:
        for j in range(4):
            s[j] = s[j] + part[g + j]
        for j in range(4):
            s[j] = s[j] + part[g + 4 + j]
        g += 8
    while g < groups:
        s[0] = s[0] + part[g]
        g += 1
    return (s[0] + s[1]) + (s[2] + s[3])


def restate_wgrad(x, dy, ksize, row, mut=None):
    """dW [cout,128,k,k] float32 the way run_wgrad computes it (form, steps and slices from H.wgrad_plan), optionally with one seeded
    fault `mut`."""
    b, h, w, c = x.shape
    cout = dy.shape[3]
    pix = b * h * w
    taps = [(ty, tx) for ty in (-1, 0, 1) for tx in (-1, 0, 1)] if ksize == 3 else [(0, 0)]
    form, steps, gx = H.wgrad_plan(pix, w, len(taps), row)
    pp = gx * steps * 64
    xf = np.asarray(x, np.float32).reshape(pix, c)
    q = np.arange(pp)
    valid = q < pix
    if mut == "tail":
        valid &= q != pix - 1
    if mut == "slice":
        assert gx > 1
        valid &= q != steps * 64
    qb, rem = q // (h * w), q % (h * w)
    yy, xx = rem // w, rem % w
    d = np.zeros((pp, 128), np.float32)
    if mut == "pitch":                                           # a 64-channel dy read with the 256-byte pitch of a 128-channel one
        flat = np.concatenate([np.asarray(dy, np.float32).reshape(-1), np.zeros(128 * pp, np.float32)])
        d[:, :cout] = np.where(valid[:, None], flat[(q[:, None] * 128 + np.arange(cout)[None])], 0)
    else:
        d[:pix][valid[:pix], :cout] = np.asarray(dy, np.float32).reshape(pix, cout)[valid[:pix]]

    def gather(ok, src):
        out = np.zeros((pp, c), np.float32)
        out[ok] = xf[src[ok]]
        return out

    def shifted_rows(ty):
        sy = yy + ty
        ok = valid & (sy >= 0) & (sy < h)
        if mut == "wrap" and ty == 1:                            # fy == H -> fb + 1 forgotten: the next image's top row feeds the bottom row
            ok = valid & (sy >= 0) & (q + w < pix)
        return ok, (qb * h + sy) * w

    images = {}
    if form == "tap":
        for ty, tx in taps:
            ok, base = shifted_rows(ty)
            sx = xx + tx
            inx = (sx >= 0) & (sx < w)
            if mut == "rowend" and tx == 1:
                inx = (sx >= 0) & (base + sx < pix)
            images[(ty, tx)] = gather(ok & inx, base + sx)
    else:
        for ty in (-1, 0, 1):
            ok, base = shifted_rows(ty)
            xr = gather(ok, base + xx)
            images[(ty, 0)] = xr
            nxt = np.concatenate([xr[1:], np.zeros((1, c), np.float32)])
            prv = np.concatenate([np.zeros((1, c), np.float32), xr[:-1]])
            end, start = xx == w - 1, xx == 0
            if mut == "rowend":
                end = np.zeros_like(end)
            if mut == "extra":                                   # the pixel in front of / behind a step is not loaded
                end, start = end | (q % 64 == 63), start | (q % 64 == 0)
            images[(ty, 1)] = np.where(end[:, None], 0, nxt).astype(np.float32)
            images[(ty, -1)] = np.where(start[:, None], 0, prv).astype(np.float32)
    dw = np.zeros((cout, 128, ksize, ksize), np.float32)
    d3 = d.reshape(gx, steps, 64, 128)
    for i, (ty, tx) in enumerate(taps):
        x3 = images[(ty, tx)].reshape(gx, steps, 64, c)
        part = np.zeros((gx, c, 128), np.float32)
        for s in range(steps):                                   # one accumulator per slice, a 64-pixel step at a time
            part = part + np.matmul(x3[:, s].transpose(0, 2, 1), d3[:, s])
        tot = _reduce_slices(part)                               # [ci][co]
        j = 8 - i if (mut == "mirror" and ksize == 3) else i
        val = tot[:, :cout] if mut == "transpose" else tot[:, :cout].T
        if ksize == 3:
            dw[:, :, j // 3, j % 3] = val
        else:
            dw[:, :, 0, 0] = val
    return dw


_wg = {}


def wg_ref(shape, kind, ksize=3, cout=128):
    key = (shape, kind, ksize, cout)
    if key not in _wg:
        x, dy = H.wgrad_case(shape, kind, cout)
        dw, mag, terms = H.wgrad_reference(x, dy, ksize)
        _wg[key] = (x, dy, dw, H.bound_wgrad(mag, terms))
    return _wg[key]


def test_wgrad_reference_is_the_definition():
    """The sliced-matmul reference against the literal pixel loop, 3x3 and 1x1, and the pair counts."""
    rng = np.random.default_rng(0)
    x, dy = rng.standard_normal((2, 4, 5, 3)), rng.standard_normal((2, 4, 5, 2))
    for k in (3, 1):
        dw, mag, terms = H.wgrad_reference(x, dy, k)
        e = np.zeros_like(dw)
        cnt = np.zeros(k * k, np.int64)
        for b in range(2):
            for yy in range(4):
                for xx in range(5):
                    for ky in range(k):
                        for kx in range(k):
                            sy, sx = yy + ky - k // 2, xx + kx - k // 2
                            if 0 <= sy < 4 and 0 <= sx < 5:
                                e[:, :, ky, kx] += np.outer(dy[b, yy, xx], x[b, sy, sx])
                                cnt[ky * k + kx] += 1
        assert np.allclose(dw, e, rtol=1e-13, atol=1e-13) and np.array_equal(cnt, terms) and (mag >= np.abs(dw) - 1e-12).all()


def test_conv_reference_is_the_definition_and_the_adjoint():
    """Forward against the pixel loop; the data gradient is the adjoint: <conv(x, w), dy> == <x, dgrad(dy, w)>."""
    rng = np.random.default_rng(1)
    x, w, dy = rng.standard_normal((2, 4, 5, 3)), rng.standard_normal((2, 3, 3, 3)), rng.standard_normal((2, 4, 5, 2))
    y, mag, t = H.conv_reference(x, w)
    e = np.zeros_like(y)
    for yy in range(4):
        for xx in range(5):
            for ky in range(3):
                for kx in range(3):
                    sy, sx = yy + ky - 1, xx + kx - 1
                    if 0 <= sy < 4 and 0 <= sx < 5:
                        e[:, yy, xx] += x[:, sy, sx] @ w[:, :, ky, kx].T
    assert np.allclose(y, e, rtol=1e-13, atol=1e-13) and t == 27 and (mag >= np.abs(y) - 1e-12).all()
    dx, _, t2 = H.conv_reference(dy, w, transposed_dgrad=True)
    assert t2 == 18 and abs((y * dy).sum() - (x * dx).sum()) < 1e-10
    dw, _, _ = H.wgrad_reference(x, dy, 3)
    assert abs((y * dy).sum() - (dw * w).sum()) < 1e-10


def test_wgrad_plan_restates_the_thresholds():
    assert H.wgrad_plan(159999, 401, 9, None)[0] == "tap" and H.wgrad_plan(160000, 400, 9, None)[0] == "row"
    assert H.wgrad_plan(252, 12, 9, True)[0] == "tap"            # NARROW: the row request falls back
    assert H.wgrad_plan(688128, 832, 9, False)[1] == 42 and H.wgrad_plan(692224, 832, 9, False)[1:] == (45, 241)
    assert H.wgrad_plan(692224, 832, 9, True) == ("row", 138, 79) and H.wgrad_plan(140800, 176, 1, None) == ("tap", 9, 245)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", H.WGRAD_SMALL)
def test_wgrad_restatement_within_bound(shape, kind):
    x, dy, ref, bound = wg_ref(shape, kind)
    for row in (False, True):
        r = H.worst(restate_wgrad(x, dy, 3, row), ref, bound)
        note(("wgrad3x3", "row" if H.wgrad_plan(x.shape[0] * x.shape[1] * x.shape[2], shape[2], 9, row)[0] == "row" else "tap", kind), r)
        assert r <= 1.0, (shape, row, r)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cout", [128, 64])
@pytest.mark.parametrize("shape", H.WGRAD_ONE_TAP)
def test_one_tap_restatement_within_bound(shape, cout, kind):
    x, dy, ref, bound = wg_ref(shape, kind, 1, cout)
    r = H.worst(restate_wgrad(x, dy, 1, False), ref, bound)
    note(("wgrad1x1", cout, kind), r)
    assert r <= 1.0, r


@pytest.mark.parametrize("shape", H.WGRAD_SMALL)
def test_integer_restatement_is_bit_exact(shape):
    x, dy = H.integer_case(shape)
    ref = H.integer_reference(x, dy, 3)
    for row in (False, True):
        assert np.array_equal(restate_wgrad(x, dy, 3, row), ref)


# mutant -> (shape, forms it exists in).  (3,11,19): 627 pixels = 9 full steps + 51; the row form cuts it into 4 slices of 3 steps.
WGRAD_MUTANTS = {"tail": ((3, 11, 19), (False, True)), "slice": ((3, 11, 19), (True,)), "extra": ((3, 11, 19), (True,)),
                 "rowend": ((3, 11, 19), (False, True)), "wrap": ((3, 11, 19), (False, True)), "mirror": ((3, 11, 19), (False,)),
                 "transpose": ((3, 11, 19), (False,))}


@pytest.mark.parametrize("mut", sorted(WGRAD_MUTANTS))
def test_wgrad_mutants_fail(mut):
    """Every seeded fault fails BOTH checks on the small case: the per-element bound on random data and bit equality on integers."""
    shape, rows = WGRAD_MUTANTS[mut]
    xi, dyi = H.integer_case(shape)
    iref = H.integer_reference(xi, dyi, 3)
    for kind in KINDS:
        x, dy, ref, bound = wg_ref(shape, kind)
        for row in rows:
            got = restate_wgrad(x, dy, 3, row, mut)
            assert H.worst(got, ref, bound) > 1.0, (mut, kind, row)
            OLD_PASSES[(mut, kind, "row" if row else "tap", shape)] = H.old_check_wgrad(got, ref)
    for row in rows:
        assert not np.array_equal(restate_wgrad(xi, dyi, 3, row, mut), iref), (mut, row)


def test_pitch_mutant_fails():
    """The 64-channel dy of the stacked heads read with the 128-channel pitch."""
    shape = (3, 11, 19)
    for kind in KINDS:
        x, dy, ref, bound = wg_ref(shape, kind, 1, 64)
        got = restate_wgrad(x, dy, 1, False, "pitch")
        assert H.worst(got, ref, bound) > 1.0
        OLD_PASSES[("pitch", kind, "tap", shape)] = H.old_check_wgrad(got, ref)
    xi, dyi = H.integer_case(shape, 64)
    assert not np.array_equal(restate_wgrad(xi, dyi, 1, False, "pitch"), H.integer_reference(xi, dyi, 1))


def test_single_pixel_faults_at_the_training_shape_against_the_old_tolerance():
    """At 4 x 200 x 176 (140 800 pixels) a single lost pixel -- the last one of the tensor, or the first one of the second slice -- moves
    dW by one outer product x[p + offset] dy[p]^T: the old check (largest error < 2e-3 of the largest element) is applied to exactly
    that, tap by tap, and the result recorded.  The typical element moves by 2e-4 of the maximum, a tenth of the old limit; the old
    check still trips on the few elements that pair the pixel's largest channels (0.3-0.5 % of them, up to 4.7e-3): a margin of 2.4,
    shrinking with the square root of the pixel count.  The integer case of the same shape sees one lost pixel bit for bit."""
    shape = H.WGRAD_INT_TRAIN
    b, h, w = shape
    for kind in KINDS:
        x, dy = H.wgrad_case(shape, kind)
        ref, _, _ = H.wgrad_reference(x, dy, 3, want_mag=False)
        steps = H.wgrad_plan(b * h * w, w, 9, False)[1]
        for name, p in (("tail", b * h * w - 1), ("slice", steps * 64)):
            pb, py, px = p // (h * w), p % (h * w) // w, p % w
            mutd = ref.copy()
            for ky in range(3):
                for kx in range(3):
                    sy, sx = py + ky - 1, px + kx - 1
                    if 0 <= sy < h and 0 <= sx < w:
                        mutd[:, :, ky, kx] -= np.outer(dy[pb, py, px], x[pb, sy, sx])
            OLD_PASSES[(name, kind, "tap", shape)] = H.old_check_wgrad(mutd, ref)
            change = np.abs(mutd - ref) / np.abs(ref).max()
            rel, typical, frac = change.max(), np.median(change[change > 0]), float((change >= 2e-3).mean())
            print(f"old tolerance, {name} pixel lost at {shape} {kind}: largest change {rel:.2e}, median change {typical:.2e} of the maximum "
                  f"(limit 2e-3), {frac:.2%} of the elements above the limit")
            # the typical element moves by a tenth of the old limit; only the product of the two largest channels of that pixel reaches it
            assert typical < 2e-3 / 5 and frac < 0.01 and rel < 3 * 2e-3
    xi, dyi = H.integer_case(shape)
    iref = H.integer_reference(xi, dyi, 3)
    lost = iref.copy()
    lost[:, :, 1, 1] -= np.outer(dyi[-1, -1, -1].astype(np.float32), xi[-1, -1, -1].astype(np.float32))
    assert not np.array_equal(lost, iref)


# ------------------------------------------------------------------------------------------------ BatchNorm restatement
F = np.float32


def _partials(vals, groups, ppi, n):
    """[n, C] float32 -> the double sums over rows as k_bn_partial + the double combine form them: thread (group g, pixel slot q) adds
    rows g * ppi + q + k * groups * ppi in ascending k, the LDS pass adds the ppi slots in ascending q, doubles from there on."""
    c = vals.shape[1]
    per = groups * ppi
    k = -(-max(n, 1) // per)
    pad = np.zeros((k * per, c), F)
    pad[:n] = vals[:n]
    pad = pad.reshape(k, groups, ppi, c)
    a = np.zeros((groups, ppi, c), F)
    for i in range(k):
        a = a + pad[i]
    s = np.zeros((groups, c), F)
    for qq in range(ppi):
        s = s + a[:, qq]
    return s


def restate_bn(case, kind, relu, live=None, mut=None):
    """Forward and backward of sec_bn_relu_fwd_nhwc / _bwd_nhwc in float32 numpy (no fused multiply-adds), optionally with one fault."""
    y, dz = case["y"].astype(F), case["dz"].astype(F)
    p, c = y.shape
    n = H.bn_live(p, live)
    nst = p if mut == "allrows" else n                            # rows the statistics run over
    groups, _ = H.bn_chain(p, n, c)
    ppi = 256 // (c // 8)
    nd = max(nst, 1)
    ga, be = case["gamma"].astype(F), case["beta"].astype(F)
    eps, mom = F(H.BN_EPS), F(H.BN_MOMENTUM)
    s0p, s1p = _partials(y, groups, ppi, nst), _partials(y * y, groups, ppi, nst)
    if mut == "fp32var":                                         # float all the way: group sums, mean, E[y^2] - m^2
        s0, s1 = F(0) * s0p[0], F(0) * s1p[0]
        for g in range(groups):
            s0, s1 = s0 + s0p[g], s1 + s1p[g]
        m = s0 / F(nd)
        var = np.maximum(s1 / F(nd) - m * m, F(0))
        mf, isf = m, (F(1) / np.sqrt(var + eps)).astype(F)
        var = var.astype(np.float64)
    else:
        s0, s1 = s0p.astype(np.float64).sum(0), s1p.astype(np.float64).sum(0)
        m = s0 / nd
        var = np.maximum(s1 / nd - m * m, 0.0)
        mf, isf = m.astype(F), (1.0 / np.sqrt(var + np.float64(eps))).astype(F)
    unb = var if (nd <= 1 or mut == "biased") else var * nd / (nd - 1)
    rm = (F(1) - mom) * case["running_mean"].astype(F) + mom * mf
    rv = (F(1) - mom) * case["running_var"].astype(F) + mom * unb.astype(F)
    yl, dl = y[:n], dz[:n]
    xh = (yl - mf) * isf
    zp = xh * ga + be
    z = H.round16(np.where(zp > 0, zp, F(0)) if relu else zp, kind)
    mask = (z > 0) if mut == "maskz" else (zp > 0)
    g = np.where(mask, dl, F(0)) if relu else dl
    db = _partials(g, groups, ppi, n).astype(np.float64).sum(0).astype(F)
    dg = _partials(g * xh, groups, ppi, n).astype(np.float64).sum(0).astype(F)
    if mut == "swap":
        db, dg = dg, db
    inv = F(1) / F(max(n, 1))
    dy = H.round16(ga * isf * (g - db * inv - xh * dg * inv), kind)
    return dict(z=z, mean=mf, invstd=isf, running_mean=rm, running_var=rv, dy=dy, dbeta=db, dgamma=dg)


def bn_ratios(case, kind, relu, got, live=None):
    ref = H.BnRef(case["y"], case["dz"], case["gamma"], case["beta"], H.BN_EPS, H.BN_MOMENTUM, relu, live, case["running_mean"],
                  case["running_var"], kind)
    r = ref.channel_ratios(got["mean"], got["invstd"], got["running_mean"], got["running_var"], got["dbeta"], got["dgamma"])
    r.update(ref.worst_elements(got["z"], got["dy"]))
    return r, ref


HOST_BN_CASES = ([(p, c, "plain") for c in H.BN_CHANNELS for p in H.BN_SMALL_P] + [(p, c, "plain") for p in H.BN_SWITCH_P for c in (8, 128)]
                 + [(p, H.BN_OFFSET_C, "offset") for p in H.BN_OFFSET_P] + [(H.BN_ROWS_N, c, "plain") for c in H.BN_ROWS_C])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p,c,variant", HOST_BN_CASES)
def test_bn_restatement_within_bounds_and_ambiguity_cap(p, c, variant, kind):
    case = H.bn_case(p, c, kind, variant)
    for relu in ((True, False) if p <= 2325 else (True,)):
        r, ref = bn_ratios(case, kind, relu, restate_bn(case, kind, relu))
        assert ref.ambiguous_fraction <= H.AMBIGUOUS_CAP, (ref.n_ambiguous, p, c)
        for name, v in r.items():
            note(("bn", name, kind), v)
            assert v <= 1.0, (name, v, p, c, variant, relu)


@pytest.mark.parametrize("kind", KINDS)
def test_ambiguity_cap_of_the_remaining_gpu_cases(kind):
    """The cases only the GPU test runs through the kernels (C = 256 at the switch): the condition is a property of the reference."""
    for p in H.BN_SWITCH_P:
        case = H.bn_case(p, 256, kind)
        ref = H.BnRef(case["y"], None, case["gamma"], case["beta"], H.BN_EPS, H.BN_MOMENTUM, True, None, kind=kind)
        assert ref.ambiguous_fraction <= H.AMBIGUOUS_CAP


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", H.BN_CAP_P)
def test_bn_static_capacity_restatement(p, kind):
    """live rows on a buffer of P rows: the reference, the restatement and the rule for live = 0 / 1 / P + 5."""
    case = H.bn_case(p, H.BN_CAP_C, kind)
    for live in H.bn_cap_lives(p):
        r, ref = bn_ratios(case, kind, True, restate_bn(case, kind, True, live), live)
        assert ref.live == min(live, p) and ref.ambiguous_fraction <= H.AMBIGUOUS_CAP
        for name, v in r.items():
            assert v <= 1.0, (name, v, live)
        if live == 0:
            assert (ref.mean == 0).all() and (ref.var == 0).all() and np.allclose(ref.invstd, 1 / np.sqrt(np.float32(1e-3)))
        if live == 1:
            assert (ref.var_unb == 0).all()                      # the kernel's rule: the biased variance of a single row


def _tiny_case():
    """fp16: a channel of subnormals k 2^-24 (k = +-1..16) under gamma = 2^-10, beta = 0: every positive pre-activation is below 2^-25
    and rounds to 0 in fp16, yet is far outside its own error bound -- the one place where a mask taken from the stored z differs."""
    rng = np.random.default_rng(5)
    p, c = 2325, 16
    case = H.bn_case(p, c, "fp16")
    k = rng.integers(1, 17, (p, c)) * rng.choice([-1, 1], (p, c))
    case["y"] = (k * 2.0 ** -24).astype(F)
    case["gamma"] = np.full(c, 2.0 ** -10, F)
    case["beta"] = np.zeros(c, F)
    return case


BN_MUTANTS = ["biased", "fp32var", "allrows", "maskz", "swap"]


@pytest.mark.parametrize("mut", BN_MUTANTS)
def test_bn_mutants_fail(mut):
    failed = {}
    for kind in KINDS:
        live = None
        if mut == "maskz":
            if kind != "fp16":
                continue                                         # bf16 has fp32's exponent range: rn(zp) > 0 == zp > 0 for every normal zp
            case = _tiny_case()
        elif mut == "fp32var":
            case = H.bn_case(H.BN_SMALL_ROWS + 1, 8, kind, "offset")
        elif mut == "allrows":
            case, live = H.bn_case(4096, 16, kind), 1000
        else:
            case = H.bn_case(2325, 16, kind)
        ok, ref = bn_ratios(case, kind, True, restate_bn(case, kind, True, live), live)
        assert max(ok.values()) <= 1.0 and ref.ambiguous_fraction <= H.AMBIGUOUS_CAP, (mut, ok)
        got = restate_bn(case, kind, True, live, mut)
        r, _ = bn_ratios(case, kind, True, got, live)
        failed[kind] = {k: v for k, v in r.items() if v > 1.0}
        print(f"bn mutant {mut} {kind}: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
        e = ref.elem(0, ref.live)
        OLD_PASSES[(mut, kind, "bn", case["y"].shape)] = H.old_check_bn(
            kind, got["z"], e["z"], got["running_mean"], ref.running_mean, got["running_var"], ref.running_var, got["dgamma"], ref.dgamma,
            got["dbeta"], ref.dbeta, got["dy"], e["dy"])
        if mut == "fp32var":
            FP32VAR[kind] = (ok["invstd"], r["invstd"])
            continue
        assert failed[kind], (mut, kind, r)
    if mut == "fp32var":
        return
    want = {"biased": "running_var", "swap": "dbeta", "maskz": "dbeta", "allrows": "mean"}[mut]
    assert all(want in f for f in failed.values()), failed


FP32VAR = {}


def test_fp32_variance_mutant_is_not_caught_and_why():
    """NOT what was hoped for, recorded as measured.  The mutant keeps float all the way (group partials added in float, mean in float,
    var = fl(s1 / n) - fl(m m)) on the offset-mean case (mean 8 x / 4 x the standard deviation, 131 073 rows, C = 8).  Its error in the
    variance is the cancellation, about 2 u m^2, plus its float chain over the 512 partials; the bound on the variance is worst-case
    over the kernel's own chain, gamma_(d+1) sum y^2 / n + 2 |m| err_mean >= 3 d u m^2 with d = 258 here (d >= 9 for every shape the
    kernel takes), so a worst-case bound of this form cannot separate the two.  Measured, invstd error / bound per channel: on the
    offset channels the mutant reaches 0.02-0.04 where the faithful restatement reaches 0.001-0.01; the largest ratio of either, 0.92
    against 0.10 in bf16 and fp16 alike, sits on the all-zero channel, whose bound is the single float cast of 1 / sqrt(eps) and which
    the mutant computes with two float roundings.  What the bounds do catch on the statistics is an error beyond the kernel's own
    arithmetic (all rows instead of the live ones, a biased running variance: test_bn_mutants_fail).  The assertions here pin the
    statement: the mutant is further from the fp64 invstd than the faithful restatement, and still inside the bound."""
    if not FP32VAR:
        test_bn_mutants_fail("fp32var")
    for kind, (faithful, mutant) in FP32VAR.items():
        print(f"fp32 variance mutant {kind}: invstd error / bound {mutant:.3g}, faithful restatement {faithful:.3g}")
        assert faithful < mutant <= 1.0, (kind, faithful, mutant)


def test_old_tolerance_lets_mutants_through():
    """The max-relative checks of tests/test_gpu_train_dense.py on the same mutants.  Runs last in this file (pytest keeps file
    order); prints both lists.  As measured, the float variance is the one it lets through; the single-pixel faults it catches at
    4 x 200 x 176 through 0.3-0.5 % of the elements (test_single_pixel_faults_at_the_training_shape_against_the_old_tolerance has the
    figures)."""
    if not OLD_PASSES:                                           # run alone: collect what the mutant tests record
        for mut in sorted(WGRAD_MUTANTS):
            test_wgrad_mutants_fail(mut)
        test_pitch_mutant_fails()
        test_single_pixel_faults_at_the_training_shape_against_the_old_tolerance()
        for mut in BN_MUTANTS:
            test_bn_mutants_fail(mut)
    through = sorted(str(k) for k, v in OLD_PASSES.items() if v)
    caught = sorted(str(k) for k, v in OLD_PASSES.items() if not v)
    print("old tolerance lets through:\n  " + "\n  ".join(through))
    print("old tolerance catches:\n  " + "\n  ".join(caught))
    assert through, "the old tolerance caught every mutant: nothing to record"


def test_report_ratios():
    for k in sorted(RATIOS, key=str):
        print("restatement", k, f"{RATIOS[k]:.3f}")
