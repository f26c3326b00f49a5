"""CPU: the fp64 reference, the exact-integer operands and the per-element bounds of tests/indice_conv_fwd_helpers.py, before the GPU
tests rely on them -- the reference against the oracle, that the bounds are SOUND (a float32 numpy model of a correct kernel passes
them in three summation orders, with and without the epilogue, for every store) and that they BITE (nine seeded wrong kernels do
not pass, on Gaussian operands by the bound and on integers by np.array_equal), next to what the old tensor-maximum check lets through."""
import numpy as np
import pytest

from oracle import oracle as orc  # noqa: E402  (test infrastructure only)

import indice_conv_fwd_helpers as H

_cache = {}


def runs(mode="subm"):
    if mode not in _cache:
        _cache[mode] = H.tables(H.geom_runs(), mode)
    return _cache[mode]


# ------------------------------------------------------------------------------------------------ reference == oracle
@pytest.mark.parametrize("mode", ["subm", "s2", "k3"])
@pytest.mark.parametrize("cin,cout", [(16, 32), (5, 7)])
def test_reference_equals_oracle(mode, cin, cout):
    """The oracle accumulates in fp64 over the rulebook's pairs and returns the float32 of the sums: one rounding away."""
    tb = runs(mode)
    feat, w, scale, shift = H.random_case(cin, cout, tb, 3)
    y, a, mag, terms = H.reference(feat, w, tb["nbr_out"], scale, shift, True)
    o = orc.indice_conv(feat, w.reshape((-1, 1, 1, cin, cout)), tb["pairs"], tb["pair_num"], tb["n_out"], acc64=True)
    assert np.all(np.abs(o - a) <= 2.0 ** -24 * np.abs(a) * (1 + 1e-6) + 2.0 ** -150)
    assert np.array_equal(y, np.maximum(a * scale.astype(np.float64) + shift, 0)) and (mag >= np.abs(a) - 1e-12).all()
    assert np.array_equal(terms, cin * (tb["nbr_out"] >= 0).sum(1))
    b = np.zeros_like(a)                                      # and against the definition, pair by pair
    for k in range(tb["kvol"]):
        live = np.nonzero(tb["nbr_out"][:, k] >= 0)[0]
        b[live] += feat[tb["nbr_out"][live, k]].astype(np.float64) @ w[k].astype(np.float64)
    assert np.allclose(a, b, rtol=1e-12, atol=1e-13)


def test_reference_is_fast_enough_at_40000_rows():
    import time
    idx, shape, batch = H.geom_big()
    tb = H.cut(H.tables((idx[:40000], shape, batch), "subm"), 40000)
    feat, w, _, _ = H.random_case(64, 64, tb, 1)
    t0 = time.perf_counter()
    a, mag, terms = H.accumulate(feat, w, tb["nbr_out"])
    dt = time.perf_counter() - t0
    assert a.shape == (40000, 64) and dt < 10.0, dt           # a second or two on an idle machine; the limit allows for a busy one


@pytest.mark.parametrize("mode", ["subm", "s2", "k3"])
@pytest.mark.parametrize("cin,cout", [(32, 32), (4, 16), (5, 7), (128, 128)])
def test_exact_case_is_exact(mode, cin, cout):
    tb = runs(mode)
    feat, w, scale, shift, a, mag, terms = H.exact_case(cin, cout, tb)
    assert ((feat != 0).sum(1) == 2).all() and set(np.unique(feat)) == {-2, -1, 0, 1, 2} and set(np.unique(w)) == {-1, 0, 1}
    assert set(np.unique(scale)) <= {-2, -1, 1, 2} and (scale < 0).any() and (scale > 0).any() and np.abs(shift).max() <= 4
    assert mag.max() <= 108 and a.any()
    if cin == cout:                                           # asymmetric: neither the offset mirror nor the transpose is invisible
        assert not np.array_equal(w, w[::-1]) and not np.array_equal(w, w.transpose(0, 2, 1))
    for epi in H.EPILOGUES:
        c = H.Case(cin, cout, tb, "bf16", True)
        y = c.y(epi)
        assert np.abs(y).max() <= 256
        for kind in ("bf16", "fp16"):                         # representable: the 16-bit store changes nothing
            assert np.array_equal(H.rnd(y, kind), y)


# ------------------------------------------------------------------------------------------------ a numpy model of the kernels
FAULTS = {"drop": "the (row, offset) contribution of smallest magnitude dropped", "mirror": "offsets mirrored (K-1-k)",
          "transpose": "W[k] transposed (square shape)", "halves": "the two 8-channel halves of every 16-channel step swapped",
          "rotate": "output channels of each 32-column slice rotated by 4", "relu_first": "ReLU before the affine map (negative scales)",
          "shift_first": "shift applied before scale", "truncate": "16-bit store truncates instead of rounding to nearest",
          "garbage_row": "a row past the live count computed from garbage"}
OLD_MUST_PASS = ("drop", "truncate")                       # what the tensor-maximum check is shown to let through
SENTINEL = -512.0                                         # what a static-capacity output holds before the launch (model only)


def smallest_contribution(feat, w, nbr):
    """(o, k) of the live pair whose contribution feat[nbr[o][k]] @ W[k] has the smallest non-zero L1 norm in the tensor."""
    best, where = np.inf, None
    for k in range(nbr.shape[1]):
        live = np.nonzero(nbr[:, k] >= 0)[0]
        if len(live):
            n1 = np.abs(feat[nbr[live, k]].astype(np.float64) @ w[k].astype(np.float64)).sum(1)
            n1[n1 == 0] = np.inf
            j = int(np.argmin(n1))
            if n1[j] < best:
                best, where = n1[j], (int(live[j]), k)
    return where


def model_acc(feat, w, nbr, order, seed=0, fault=None, split=False):
    """fp32 accumulators of a kernel, [n_out, cout] float32: one rounding per term (an exact product added to an fp32 accumulator, as
    fmaf and the MFMA accumulate), the K * cin terms of an element in the order
      "seq"     offsets ascending, channels ascending, one accumulator;
      "splitk"  four accumulators (offset k goes to k % 4: the four waves of k_conv_mfma_sk), reduced pairwise (1 -> 0, 3 -> 2, 2 -> 0);
      "random"  a random permutation of all terms.
    split: fp32 operands as two bf16 halves, the lo * lo product dropped (k_conv_rows_x3_f32)."""
    rng = np.random.default_rng(seed)
    K, cin, cout = w.shape
    n_in = len(feat)
    nbr = nbr.copy()
    if fault == "drop":
        o, k = smallest_contribution(feat, w, nbr)
        nbr[o, k] = -1
    f0 = np.concatenate([feat.astype(np.float64), np.zeros((1, cin))])
    w64 = w.astype(np.float64)
    if split:
        hi = lambda v: H.rnd(v, "bf16").astype(np.float64)
        fh, wh = hi(f0), hi(w64)
        fl, wl = hi(f0 - fh), hi(w64 - wh)
    idx = np.where(nbr >= 0, nbr, n_in)
    terms = [(k, ci) for k in range(K) for ci in range(cin)]
    if order == "random":
        terms = [terms[j] for j in rng.permutation(len(terms))]
    accs = np.zeros((4 if order == "splitk" else 1, len(nbr), cout), np.float32)
    for k, ci in terms:
        kw = K - 1 - k if fault == "mirror" else k
        cf = ci ^ 8 if fault == "halves" else ci
        wrow = (lambda m: m[kw][:, ci] if fault == "transpose" else m[kw][ci])
        if split:
            x_h, x_l = fh[idx[:, k], cf][:, None], fl[idx[:, k], cf][:, None]
            prod = x_h * wrow(wh)[None, :] + x_h * wrow(wl)[None, :] + x_l * wrow(wh)[None, :]
        else:
            prod = f0[idx[:, k], cf][:, None] * wrow(w64)[None, :]
        s = k % 4 if order == "splitk" else 0
        accs[s] = (accs[s].astype(np.float64) + prod).astype(np.float32)
    if order == "splitk":
        return (accs[0] + accs[1]) + (accs[2] + accs[3])      # float32 additions: one rounding each
    return accs[0]


def model_store(x, store, truncate=False):
    x = np.asarray(x, np.float32)
    if store == "fp32":
        return x
    if not truncate:
        return H.rnd(x, store)
    if store == "bf16":
        return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float32)


def model_epilogue(acc, scale, shift, relu, store, fault=None):
    """epilogue_v in float32 (a rounded product, then a rounded sum), ReLU, one store."""
    v = np.asarray(acc, np.float32)
    if fault == "rotate":
        v = np.concatenate([np.roll(v[:, c:c + 32], -4, axis=1) for c in range(0, v.shape[1], 32)], 1)
    if fault == "relu_first" and relu:
        v = np.maximum(v, np.float32(0))
    if fault == "shift_first" and shift is not None and scale is not None:
        v = (v + shift.astype(np.float32)) * scale.astype(np.float32)
    else:
        if scale is not None:
            v = v * scale.astype(np.float32)
        if shift is not None:
            v = v + shift.astype(np.float32)
    if relu and fault != "relu_first":
        v = np.maximum(v, np.float32(0))
    return model_store(v, store, fault == "truncate")


def model_kernel(c, epi, store, order, seed=0, fault=None, live=None):
    """The model on a Case.  live: a static-capacity launch -- the table is padded with GARBAGE rows, the output starts as SENTINEL,
    the kernel writes rows [0, live); the "garbage_row" fault also writes row `live`, from table entries taken modulo n_in."""
    nbr = c.tb["nbr_out"]
    split = c.kind == "fp32_split"
    scale, shift, relu = c.vectors(epi)
    if live is None:
        return model_epilogue(model_acc(c.feat, c.w, nbr, order, seed, fault, split), scale, shift, relu, store, fault)
    out = np.full((len(nbr), c.cout), SENTINEL, np.float32)
    rows = live + (1 if fault == "garbage_row" else 0)
    table = np.concatenate([nbr[:live], np.full((len(nbr) - live, nbr.shape[1]), H.GARBAGE, np.int32)])
    table[live:] %= c.tb["n_in"]
    out[:rows] = model_epilogue(model_acc(c.feat, c.w, table[:rows], order, seed, fault, split), scale, shift, relu, store, fault)
    return out


def expected(c, epi, bound_kind, store, live=None):
    """(y, bound) of the whole output buffer; rows from `live` on keep the SENTINEL (bound: the floor alone)."""
    y, b = c.y(epi), c.bound(epi, bound_kind, store)
    if live is not None:
        y, b = y.copy(), b.copy()
        y[live:], b[live:] = SENTINEL, 1e-30
    return y, b


@pytest.fixture(scope="module")
def gauss():
    return {kind: H.Case(32, 32, runs(), kind, False) for kind in ("bf16", "fp16", "fp32_split", "fp32_exact")}


@pytest.fixture(scope="module")
def exact():
    return H.Case(32, 32, runs(), "bf16", True)


# ------------------------------------------------------------------------------------------------ the bounds are sound
@pytest.mark.parametrize("order", ["seq", "splitk", "random"])
@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp32_split", "fp32_exact"])
def test_bounds_pass_a_correct_kernel(gauss, exact, kind, order):
    """Every summation order x no epilogue / scale + shift + ReLU (negative scales) / each flag alone x every store of the kind."""
    c = gauss[kind]
    bkind = kind
    stores = ("fp32",) if kind.startswith("fp32") else (kind, "fp32")
    acc = model_acc(c.feat, c.w, c.tb["nbr_out"], order, 1, None, kind == "fp32_split")
    worst_seen = 0.0
    for epi in H.EPILOGUES:
        scale, shift, relu = c.vectors(epi)
        for store in stores:
            out = model_epilogue(acc, scale, shift, relu, store)
            r = H.worst(out, c.y(epi), c.bound(epi, bkind, store))
            worst_seen = max(worst_seen, r)
            assert r <= 1.0, (kind, order, epi, store, r)
    assert worst_seen > 0.01, worst_seen                      # the bound is not orders of magnitude loose either
    if kind in ("bf16", "fp16"):
        eacc = model_acc(exact.feat, exact.w, exact.tb["nbr_out"], order, 2)
        for epi in H.EPILOGUES:                               # integers: bit for bit in any order
            assert np.array_equal(model_epilogue(eacc, *exact.vectors(epi), kind), exact.y(epi))


def test_static_capacity_model_passes(gauss, exact):
    for live in (0, 1, 33, runs()["n_out"] - 1):
        y, b = expected(gauss["bf16"], "full", "bf16", "bf16", live)
        assert H.worst(model_kernel(gauss["bf16"], "full", "bf16", "splitk", 3, live=live), y, b) <= 1.0
        assert np.array_equal(model_kernel(exact, "full", "bf16", "splitk", 3, live=live), expected(exact, "full", "bf16", "bf16", live)[0])


# ------------------------------------------------------------------------------------------------ the bounds bite
@pytest.mark.parametrize("fault", list(FAULTS))
def test_bounds_bite(gauss, exact, fault, capsys):
    """Each wrong kernel of FAULTS, modelled on `runs` (SubM, 32 -> 32, bf16 store, scale + shift + ReLU with negative scales), misses
    the per-element bound on the Gaussian case AND differs from the exact-integer case under np.array_equal -- with ONE exception that
    arithmetic forces: the truncating store cannot show on integers the format holds exactly (truncation and rounding agree on them, and
    the exact case is exact BECAUSE every result is representable); the bound on Gaussian operands is what catches it, and that is what
    is asserted for it.

    The old check (tests/test_gpu_parity.py::test_indice_conv_half_mfma: rtol = atol / max|ref| = 2^-7 for bf16) is evaluated on the
    same outputs: it must let the dropped small contribution and the truncating store through (asserted); what it does with the
    others is printed."""
    c, live = gauss["bf16"], 400 if fault == "garbage_row" else None
    y, b = expected(c, "full", "bf16", "bf16", live)
    out = model_kernel(c, "full", "bf16", "splitk", 1, fault, live)
    ratio, old = H.worst(out, y, b), H.old_forward_check(out, y, "bf16")
    good = model_kernel(c, "full", "bf16", "splitk", 1, None, live)
    assert H.worst(good, y, b) <= 1.0 and H.old_forward_check(good, y, "bf16")
    ey = expected(exact, "full", "bf16", "bf16", live)[0]
    same = np.array_equal(model_kernel(exact, "full", "bf16", "splitk", 2, fault, live), ey)
    with capsys.disabled():
        print(f"\n  {fault}: {FAULTS[fault]}: error / bound {ratio:.3g} (caught), integers {'EQUAL' if same else 'differ (caught)'}, "
              f"old tensor-maximum check {'PASSES' if old else 'fails'}")
    assert ratio > 1.0, (fault, ratio)
    assert same == (fault == "truncate"), fault
    if fault in OLD_MUST_PASS:
        assert old, fault
    if fault == "drop":                                       # the dropped contribution alone, element by element
        o, k = smallest_contribution(c.feat, c.w, c.tb["nbr_out"])
        wrong = np.nonzero((np.abs(out.astype(np.float64) - y) > b).any(1))[0]
        assert list(wrong) == [o], (wrong, o)


def test_bounds_bite_on_the_fp16_and_fp32_stores(gauss):
    """The same dropped contribution under the fp16 store and the two fp32 arithmetics; the truncating fp16 store."""
    for kind, store in (("fp16", "fp16"), ("fp32_split", "fp32"), ("fp32_exact", "fp32")):
        c = gauss[kind]
        out = model_kernel(c, "full", store, "seq", 1, "drop")
        assert H.worst(out, c.y("full"), c.bound("full", kind, store)) > 1.0, kind
    c = gauss["fp16"]
    out = model_kernel(c, "full", "fp16", "seq", 1, "truncate")
    assert H.worst(out, c.y("full"), c.bound("full", "fp16", "fp16")) > 1.0 and H.old_forward_check(out, c.y("full"), "fp16")
