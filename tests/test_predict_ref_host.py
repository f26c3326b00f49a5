"""The references of tests/predict_ref_helpers.py against what the project already holds from the executed reference, and the
comparison function of tests/test_gpu_predict_edges.py against planted mistakes (no GPU needed).

- decode_reference64 vs dec_enc / dec_anchors / dec_out of the torch-modules golden file: within one fp32 rounding per output
  operation of the float32 reference (the bounds of decode_bounds(), which the GPU test applies to the kernel).
- the limit_period lines of finalize_reference32 vs lp_val / lp_out, bit for bit.
- select_reference vs torch.topk on tie-free fp32 scores and vs the ordering rule of oracle/cpu_forward.py.
- a torch emulation of the select with one mistake planted at a time: check_selection must fail for each.
- every input the GPU select tests list keeps the threshold band (checked here, on the CPU, before any GPU run).
"""
import math

import numpy as np
import pytest
import torch

import predict_ref_helpers as R


def test_decode_reference64_matches_the_recorded_second_box_decode(golden):
    g = golden("torch_modules")
    e, a = torch.from_numpy(g["dec_enc"]), torch.from_numpy(g["dec_anchors"])
    ref = R.decode_reference64(e, a)
    # the recorded output is torch's float32 evaluation: each of its outputs carries the roundings decode_bounds() counts
    ok, ratio = R.within(torch.from_numpy(g["dec_out"]), ref, R.decode_bounds(e, a, ref))
    assert ok, ratio
    assert ratio > 0.01, "the recorded outputs differ from float64 by their float32 roundings: a zero difference means the test compares nothing"


def test_limit_period_lines_are_the_recorded_limit_period_bit_for_bit(golden):
    g = golden("torch_modules")
    out = R.limit_period_f32(g["lp_val"], 1.0, np.float32(np.pi))
    assert out.dtype == np.float32 and R.same_bits_f32(out, g["lp_out"])
    # finalize_reference32 with offset 0, limit offset 1, ONE bin of period fl32(pi)... does not exist (bins divide 2 pi); with two bins the
    # period is fl32(2 pi) / 2 = fl32(pi) exactly, so its rotation column for direction label 0 is the same five lines
    assert np.float32(6.283185307179586) / np.float32(2) == np.float32(np.pi)
    n = g["lp_val"].shape[0]
    dec = np.zeros((1, n, 7), np.float32)
    dec[0, :, 6] = g["lp_val"]
    fin = R.finalize_reference32(dec, np.zeros((1, n), np.float32), np.zeros((1, n), np.int32), np.zeros((1, n), np.int32),
                                 np.arange(n)[None], np.array([n]), n, 1, 0.0, 1.0, 2, None)
    assert R.same_bits_f32(fin["boxes"][0, :, 6], g["lp_out"]) and fin["valid"].all()


def _tie_free_logits(b, n, nc, seed):
    """fp32 logits on a shuffled grid coarse enough (>= 7e-5 apart in [-5, 1.5]) that their fp32 sigmoids are all distinct."""
    g = torch.Generator().manual_seed(seed)
    total = b * n * nc
    assert total <= 90000
    return torch.linspace(-5.0, 1.5, total)[torch.randperm(total, generator=g)].reshape(b, n, nc)


@pytest.mark.parametrize("nc", [1, 3])
def test_select_reference_is_topk_on_tie_free_scores(nc):
    b, n, k, thr = 2, 9001, 1000, 0.05
    x = _tie_free_logits(b, n, nc, nc)
    ref = R.select_reference(x, k, thr)
    scores = torch.sigmoid(x).max(-1)
    for f in range(b):
        # voxelnet.py:551-570: threshold mask, then topk of the surviving scores
        keep = scores.values[f] >= thr
        ids = torch.nonzero(keep).squeeze(1)
        top = torch.topk(scores.values[f][ids], min(k, ids.numel()))
        assert int(ref["counts"][f]) == top.indices.numel() > 0
        assert torch.equal(ref["idx"][f], ids[top.indices])
        assert torch.equal(ref["label"][f], scores.indices[f][ids[top.indices]])
        np.testing.assert_allclose(ref["score64"][f].numpy(), top.values.double().numpy(), rtol=2.0 ** -22)
    assert ref["margin"] > 0


def test_select_reference_follows_the_cpu_forward_ordering_rule():
    """oracle/cpu_forward.py: keep = score >= thr, then argsort(-score, stable) -- descending score, ties by ascending anchor index.
    On 16-bit-valued logits (heavy ties; distinct values far enough apart that their fp32 sigmoids stay distinct) that is the order of
    select_reference."""
    g = torch.Generator().manual_seed(3)
    b, n, k, thr = 2, 5000, 300, 0.3
    x = (torch.randn(b, n, 1, generator=g) * 1.5 - 1.0).bfloat16().float()
    x = R.redraw_band(x, thr)
    ref = R.select_reference(x, k, thr)
    for f in range(b):
        cls = torch.sigmoid(x[f, :, 0])
        keep = cls >= thr
        sel_all = torch.nonzero(keep).squeeze(1)
        order = torch.argsort(-cls[sel_all], stable=True)[:min(k, int(keep.sum()))]
        assert torch.equal(ref["idx"][f], sel_all[order]) and int(ref["counts"][f]) == order.numel()
    assert ref["margin"] >= R.BAND


# ---------------------------------------------------------------------------------------------------------------- planted mistakes
def _emulated_select(x, k, thr, mistake=None):
    """The select in the kernels' output layout ([B, k] rows, counts), written independently of select_reference (float keys, two-key
    lexsort), with one mistake at a time."""
    b, n, c = x.shape
    k = min(k, n, 1024)
    top_idx = torch.zeros(b, k, dtype=torch.int32)
    top_score = torch.zeros(b, k)
    top_label = torch.zeros(b, k, dtype=torch.int32)
    counts = torch.zeros(b, dtype=torch.int32)
    thr32 = np.float32(thr)
    for f in range(b):
        v = x[f].numpy().astype(np.float32)
        nan = np.isnan(v).any(1)
        vv = np.where(np.isnan(v), -np.inf, v)
        best = vv.max(1)
        eq = vv == best[:, None]
        label = (c - 1 - np.argmax(eq[:, ::-1], 1)) if mistake == "last_label" else np.argmax(eq, 1)
        best = vv[np.arange(n), label]
        # float order with -0.0 below +0.0: a second key of the sign bit
        signbit = np.signbit(best).astype(np.int64)
        idx = np.arange(n)
        alive = ~nan
        if mistake == "nan_first":
            best = np.where(nan, np.inf, best)
            alive = np.ones(n, bool)
        if mistake == "chunk_drop":
            alive = alive & (idx != 8192)
        tie = -idx if mistake == "ties_desc" else idx
        order = np.lexsort((tie, signbit, -best.astype(np.float64)))
        order = order[alive[order]][:k]
        with np.errstate(over="ignore"):
            score = (np.float32(1) / (np.float32(1) + np.exp(-best.astype(np.float32)))).astype(np.float32)
        score = np.where(nan, np.float32(np.nan), score)
        ok = score[order] > thr32 if mistake == "gt_threshold" else score[order] >= thr32
        m = order.size
        top_idx[f, :m] = torch.from_numpy(order.astype(np.int32))
        top_score[f, :m] = torch.from_numpy(score[order])
        top_label[f, :m] = torch.from_numpy(label[order].astype(np.int32))
        counts[f] = int(ok.sum())
    return top_idx, top_score, top_label, counts


def _planted_input():
    """A trained-like head (fewer than k candidates: the threshold decides counts) with ties, class ties, exact +-0.0 with thr = 0.5,
    a NaN, and anchor 8192 (first of the second chunk) in the selection."""
    n, nc = 9000, 3
    x = R.make_logits("trained", 2, n, nc, 0.5, torch.bfloat16, 11).float()
    x[:, 400:420, 1] = 1.0                             # twenty anchors tied on one value
    x[:, 8192, :] = 3.0                                # in the selection whatever the ties do
    x[:, 100:140:2, :] = 0.0                           # exactly on the threshold: sigmoid(+-0) = 0.5
    x[:, 101:140:2, :] = -0.0
    x[:, 200:260, 0] = 0.5                             # equal maxima in two classes: the first wins
    x[:, 200:260, 1] = -1.0
    x[:, 200:260, 2] = 0.5
    x[0, 300, 0] = math.nan
    x[1, 301, 2] = -math.nan
    return x


def test_the_emulation_without_a_mistake_passes_the_comparison():
    x = _planted_input()
    ref = R.select_reference(x, 1000, 0.5)
    assert ref["margin"] >= R.BAND and 100 < int(ref["counts"].min()) and int(ref["counts"].max()) < 1000
    R.check_selection(_emulated_select(x, 1000, 0.5), ref)


@pytest.mark.parametrize("mistake", ["ties_desc", "last_label", "gt_threshold", "nan_first", "chunk_drop"])
def test_each_planted_mistake_fails_the_comparison(mistake):
    x = _planted_input()
    ref = R.select_reference(x, 1000, 0.5)
    with pytest.raises(AssertionError):
        R.check_selection(_emulated_select(x, 1000, 0.5, mistake), ref)


# ---------------------------------------------------------------------------------------------------------------- the threshold band
def test_every_listed_select_input_keeps_the_threshold_band():
    """Condition of the GPU tests: |score64 - float32(thr)| >= 2^-20 for every anchor not exactly on the threshold, so that the device's
    comparison (its sigmoid is within 2^-22) decides every anchor as the reference does.  The same generators, seeds and cases."""
    def margin(x, thr):
        s = torch.sigmoid(x.double())
        t = float(np.float32(thr))
        off = s != t
        if not bool(off.any()):
            return math.inf
        return float((s[off] - t).abs().min())

    for i, (dtype, n, nc, b) in enumerate(R.boundary_cases()):
        for p, pattern in enumerate(R.PATTERNS):
            x = R.make_logits(pattern, b, n, nc, 0.3, dtype, 100 * i + p)
            assert margin(x, 0.3) >= R.BAND, (dtype, n, nc, pattern)
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for n in (8193, 1001):
            for thr in (0.0, 0.05, 0.5, 0.9):
                x = R.k_thr_logits(n, thr, dtype, 17)
                assert margin(x, thr) >= R.BAND, (dtype, n, thr)
                on = torch.sigmoid(x.double()) == float(np.float32(thr))
                assert (thr == 0.5 and bool((x[on] == 0).all()) and int(on.sum()) == 80) or not bool(on.any())


def test_select_form_is_the_library_decision():
    """select_form() (written from the documented table) against predict_select_decide through sec_predict_select_plan_name, a host-only
    query: name and chunk count, all three dtypes, every listed boundary and its neighbours, and a seeded sample up to 6 M anchors."""
    from second_amd import ops
    ns = {m for n in R.BOUNDARY_N + R.BOUNDARY_N_HUGE + R.BOUNDARY_N_FP32 for m in (n - 1, n, n + 1)}
    ns |= {int(n) for n in np.random.default_rng(5).integers(1, 6_000_001, 4000)}
    seen = set()
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for n in sorted(ns):
            assert ops.predict_select_plan(n, dtype) == R.select_form(n, dtype), (n, dtype)
            seen.add(R.select_form(n, dtype)[0])
    assert seen == {"direct", "radix16", "radix32"} | {"chunk%d+kp%d" % (c, k) for c in (4, 36) for k in (5, 10, 20, 36)}
    from second_amd import runtime as rt
    assert rt.lib().sec_predict_select_plan_name(8193, 3, None) == b"" and rt.lib().sec_predict_select_plan_name(8193, -1, None) == b""


def test_the_form_table_boundaries():
    """select_form() restates predict_select_launch's decision; the boundary list of the GPU test sits on every edge of it."""
    f = lambda n, dt=torch.bfloat16: R.select_form(n, dt)[0]
    assert [f(n) for n in (1, 8192)] == ["direct"] * 2 and f(8193) == "chunk4+kp5" and R.select_form(16385, torch.float16) == ("chunk4+kp5", 3)
    assert (f(81920), f(81921), f(163840), f(163841), f(327680), f(327681)) == ("chunk4+kp5", "chunk4+kp10", "chunk4+kp10", "chunk4+kp20",
                                                                                 "chunk4+kp20", "chunk4+kp36")
    assert (f(589824), f(589825), f(5308416), f(5308417)) == ("chunk4+kp36", "chunk36+kp5", "chunk36+kp36", "radix16")
    assert f(70401, torch.float32) == "radix32"
    forms = {R.select_form(n, dt)[0] for dt, n, _, _ in R.boundary_cases()}
    assert forms == {"direct", "chunk4+kp5", "chunk4+kp10", "chunk4+kp20", "chunk4+kp36", "chunk36+kp5", "chunk36+kp36", "radix16", "radix32"}
    for n in R.BOUNDARY_N + R.BOUNDARY_N_FP32 + R.BOUNDARY_N_HUGE:
        a, h, w = R.factor_ahw(n)
        assert a * h * w == n and (w & (w - 1) != 0 or n & (n - 1) == 0 or w == n), (n, a, h, w)
