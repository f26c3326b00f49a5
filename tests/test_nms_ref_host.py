"""The references of tests/nms_ref_helpers.py against what the project holds from the executed reference and against the fp32 oracle, the
comparison functions of tests/test_gpu_nms_edges.py against planted mistakes, and the conditions on that file's inputs (no GPU needed).

- rect_inter64 / iou64 vs tests/golden/rotate_iou.npz within iou_bound, all four criteria; greedy_nms64 vs rotate_nms.npz and
  nms_axis_aligned.npz exactly (both semantics, eps 0 and 1); greedy_nms64 vs the fp32 oracle on every decision input of the GPU file.
- the constant of the bound: C0 re-measured on the oracle over the IoU-matrix inputs stays within the recorded value.
- the exact-threshold pairs give an IoU bit-equal to the threshold on the oracle; numba semantics keep both boxes, cpu semantics drop one.
- eight mistakes planted in a copy of the greedy loop / the IoU functions fail check_keep / check_iou_matrix on the GPU tests' own inputs.
- caps: at most 2 % of the pairs of an IoU-matrix input are outside general position; no consulted pair of a decision input lies inside
  its band, and at most 5 % of the two-box frames were filtered away for it.
"""
import ctypes

import numpy as np
import pytest

import nms_ref_helpers as R
from oracle import oracle as orc  # noqa: E402  (test infrastructure only)

SEMANTICS = ("numba", "cpu")
KINDS = ("rotate", "axis_aligned")


def _oracle_nms(kind, d, thr, sem, eps=1.0, post=0):
    k = orc.rotate_nms_sorted(d, thr, sem) if kind == "rotate" else orc.nms_sorted(d, thr, sem, eps)
    return k[:post] if post else k


# ---------------------------------------------------------------------------------------------------------------- recorded outputs
@pytest.mark.parametrize("crit", [-1, 0, 1, 2])
def test_iou64_matches_the_recorded_rotate_iou_within_the_bound(golden, crit):
    g = golden("rotate_iou")
    b, q = g["boxes"][:, None], g["qboxes"][None]
    ref = R.iou_matrix64(g["boxes"], g["qboxes"], crit)
    gp = R.general_position(b, q)
    assert gp.mean() > 0.98
    err = np.abs(g[f"iou_c{crit}"] - ref)[gp] / R.iou_bound(b, q, crit)[gp]
    assert err.max() <= 1.0, err.max()
    assert err.max() > 0.01, "the recorded values carry float32 roundings: a zero difference means nothing was compared"
    # the asymmetric criteria are told apart: swapped, the recorded values miss the bound
    if crit in (0, 1):
        swapped = R.iou_matrix64(g["boxes"], g["qboxes"], 1 - crit)
        assert (np.abs(g[f"iou_c{crit}"] - swapped)[gp] / R.iou_bound(b, q, 1 - crit)[gp]).max() > 1.0
    if crit == -1:
        a, bb = g["special_a"], g["special_b"]
        ok = R.general_position(a, bb)
        assert ok.sum() >= 3
        assert (np.abs(g["special_iou"] - R.iou64(a, bb))[ok] <= R.iou_bound(a, bb)[ok]).all()
        np.testing.assert_allclose(R.iou64(a[:3], bb[:3]), [1.0, 1.0 / 3.0, 1.0 / np.sqrt(2.0)], rtol=1e-7)    # known answers, geometry only


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
@pytest.mark.parametrize("thr", [0.01, 0.3])
def test_greedy_nms64_gives_the_recorded_rotate_nms_keep_lists(golden, tag, thr):
    g = golden("rotate_nms")
    dets = g[f"dets_{tag}"]
    order = dets[:, 5].argsort()[::-1]
    for sem in SEMANTICS:
        keep, band = R.greedy_nms64(dets[order], thr, "rotate", sem)
        np.testing.assert_array_equal(order[keep], g[f"keep_{tag}_{thr}"])
        assert keep.dtype == np.int32 and (band > 0 or len(dets) == 1)


@pytest.mark.parametrize("thr", [0.1, 0.5])
def test_greedy_nms64_gives_the_recorded_axis_aligned_keep_lists(golden, thr):
    g = golden("nms_axis_aligned")
    dets = g["dets"]
    order = dets[:, 4].argsort()[::-1]
    for sem, eps, name in (("numba", 1.0, "keep_gpu"), ("numba", 0.0, "keep_gpu"), ("cpu", 0.0, "keep_jit_eps0"), ("cpu", 1.0, "keep_jit_eps1")):
        keep, _ = R.greedy_nms64(dets[order], thr, "axis_aligned", sem, eps)          # numba: the +1 convention whatever eps says
        np.testing.assert_array_equal(order[keep], g[f"{name}_{thr}"])
    assert not np.array_equal(g[f"keep_jit_eps0_{thr}"], g[f"keep_jit_eps1_{thr}"]), "the recorded lists tell the conventions apart"


def test_aa_iou64_is_the_oracle_formula_within_aa_bound():
    rng = np.random.default_rng(5)
    xy, wh = rng.uniform(0, 60, (200, 2)), rng.uniform(2, 25, (200, 2))
    d = np.ascontiguousarray(np.concatenate([xy, xy + wh], 1), np.float32)
    for eps in (0.0, 1.0):
        got = np.zeros((200, 200), np.float32)
        orc.lib().orc_standup_iou(orc._fp(d), 200, ctypes.c_float(eps), orc._fp(got))          # box_np_ops.iou_jit restated in fp32
        ref, bound = R.aa_iou64(d[:, None], d[None], eps), R.aa_bound(d[:, None], d[None], eps)
        ratio = (np.abs(got - ref) / bound).max()
        assert 0.001 < ratio <= 1.0, ratio


# ---------------------------------------------------------------------------------------------------------------- the constant
def test_recorded_c0_covers_the_oracle_on_every_iou_matrix_input_and_the_inputs_are_fair():
    worst, where, pairs = 0.0, None, 0
    for gen, n, k in R.iou_matrix_cases():
        b, q = R.iou_matrix_input(gen, n, k)
        gp = R.general_position(b[:, None], q[None])
        assert 1.0 - gp.mean() <= 0.02, (gen, n, k, 1.0 - gp.mean())                                  # the cap of the issue
        inter = R.rect_inter64(b[:, None], q[None])
        assert (inter[gp] > 0).sum() >= 1, (gen, n, k)
        if n * k >= 64:
            assert 0.03 <= (inter > 0).mean() <= 0.3, (gen, n, k, (inter > 0).mean())
            assert R.iou64(b[-1], q[-1]) == 1.0 and b[-1, 4] == 0.0                                     # the duplicate
            assert all(orc.rotate_iou(b[-1:], q[-1:], crit)[0, 0] == 1.0 for crit in (-1, 0, 1))
        ratio = (np.abs(orc.rotate_iou(b, q, 2) - inter) / R.delta_perimeter(b[:, None], q[None]))[gp].max()
        pairs += int(gp.sum())
        if ratio > worst:
            worst, where = ratio, (gen, n, k)
    print(f"[nms-ref] C0 measured {worst:.3f} at {where} over {pairs} general-position pairs; recorded {R.C0}, C = {R.C}")
    assert worst <= R.C0, (worst, where)
    assert worst >= 0.5 * R.C0, "the recorded C0 is no longer the measured one: re-measure and update the docstring and DESIGN.md"
    assert R.C == 4 * R.C0


def test_iou_matrix_comparison_accepts_the_oracle_and_rejects_swapped_criteria():
    """check_iou_matrix (the GPU test's comparison) on the oracle's fp32 values; planted mistake 8: criterion 0 and 1 swapped."""
    for gen, n, k in (("car", 63, 65), ("long", 65, 63), ("small", 64, 64), ("car", 1, 1), ("small", 129, 1), ("long", 1, 129)):
        b, q = R.iou_matrix_input(gen, n, k)
        for crit in (-1, 0, 1, 2):
            assert R.check_iou_matrix(orc.rotate_iou(b, q, crit), b, q, crit) <= 0.25 + 1e-9        # the oracle defines C0 = C / 4
        if n * k > 1:
            for crit in (0, 1):
                with pytest.raises(AssertionError):
                    R.check_iou_matrix(orc.rotate_iou(b, q, 1 - crit), b, q, crit)
    b, q = R.iou_matrix_input("car", 64, 64)
    far = orc.rotate_iou(b, q, -1)
    far[0, 1:] = np.where(far[0, 1:] == 0, 1e-30, far[0, 1:])
    with pytest.raises(AssertionError):
        R.check_iou_matrix(far, b, q, -1)


# ---------------------------------------------------------------------------------------------------------------- exact thresholds
def test_exact_pairs_sit_on_the_threshold_bit_for_bit_on_the_oracle():
    for thr, pairs in R.EXACT_ROTATED.items():
        for a, b in pairs:
            for shift in ((0.0, 0.0), (32.0, -64.0), (-1024.5, 512.25)):
                d = np.array([a, b], np.float32)
                d[:, 0] += shift[0]
                d[:, 1] += shift[1]
                assert orc.rotate_iou(d[:1], d[1:], -1)[0, 0] == np.float32(thr) == thr
                assert R.iou64(d[0], d[1]) == thr
                assert orc.rotate_nms_sorted(d, thr, "numba").tolist() == [0, 1] and orc.rotate_nms_sorted(d, thr, "cpu").tolist() == [0]
                assert R.greedy_nms64(d, thr, "rotate", "numba")[0].tolist() == [0, 1] and R.greedy_nms64(d, thr, "rotate", "cpu")[0].tolist() == [0]
                # no shared edge lines: the pair is in general position, far from the degenerate cases
                assert R.corner_edge_distance(d[0], d[1]) >= 0.25
    for (conv, thr), (a, b) in R.EXACT_AA.items():
        d = np.array([a, b], np.float32)
        eps = 1.0 if conv == "plus1" else 0.0
        assert R.aa_iou64(d[0], d[1], eps) == thr
        assert orc.nms_sorted(d, thr, "cpu", eps).tolist() == [0] and R.greedy_nms64(d, thr, "axis_aligned", "cpu", eps)[0].tolist() == [0]
        if conv == "plus1":
            assert orc.nms_sorted(d, thr, "numba").tolist() == [0, 1] and R.greedy_nms64(d, thr, "axis_aligned", "numba")[0].tolist() == [0, 1]
            assert orc.nms_sorted(d, np.nextafter(np.float32(thr), np.float32(0)), "numba").tolist() == [0]


@pytest.mark.parametrize("kind", KINDS)
def test_exact_pair_frames_put_the_pair_on_the_tile_edges(kind):
    for n in (65, 130):
        pair = R.EXACT_ROTATED[0.25][0] if kind == "rotate" else R.EXACT_AA[("plus1", 0.25)]
        dets, cols = R.exact_pair_frames(kind, pair, n, shift=(32.0, 64.0))
        assert cols.tolist() == [1, 16, 17, 64, 64, n - 1, n - 1]
        for f, col in enumerate(cols):
            assert _oracle_nms(kind, dets[f], 0.25, "numba").tolist() == list(range(n))
            assert _oracle_nms(kind, dets[f], 0.25, "cpu").tolist() == [i for i in range(n) if i != col]
            info = {}
            keep, _ = R.greedy_nms64(dets[f], 0.25, kind, "cpu", 1.0, info=info)
            assert keep.tolist() == [i for i in range(n) if i != col]


# ---------------------------------------------------------------------------------------------------------------- decision inputs
@pytest.mark.parametrize("shape", R.PAIR_SHAPES)
def test_two_box_frames_are_outside_their_bands_and_agree_with_the_oracle(shape):
    for thr in R.THRESHOLDS:
        dets, filtered = R.decision_pairs(shape, thr)
        assert dets.shape == (R.PAIR_FRAMES, 2, 5) and filtered <= 0.05, (shape, thr, filtered)
        iou = R.iou64(dets[:, 0], dets[:, 1])
        assert iou.min() == 0.0 and iou.max() > (0.9 if shape != "long" else 0.8) and iou.max() <= 0.98
        zone = (iou > thr) & (iou < 1.15 * thr + 2e-4)
        assert zone.sum() >= (300 if thr >= 0.1 else 50 if thr > 0 else 0), (shape, thr, zone.sum())     # where the screen's margin decides
        assert (np.histogram(iou, bins=np.linspace(0, 1, 11))[0][:9] >= 150).all()
        for sem in SEMANTICS:
            assert R.pair_comparable(dets, thr, sem == "cpu").all()
            want = R.pair_decisions64(dets, thr, sem)
            assert 0.02 < (want == 1).mean() < 0.98 or thr == 0.9
            for f in range(0, R.PAIR_FRAMES, 3):                      # a third of the frames on the fp32 oracle, and on the general loop
                assert orc.rotate_nms_sorted(dets[f], thr, sem).size == want[f], (shape, thr, sem, f)
            for f in range(0, R.PAIR_FRAMES, 64):
                info = {}
                keep, _ = R.greedy_nms64(dets[f], thr, "rotate", sem, info=info)
                assert keep.size == want[f] and info["ratio"] > 1.0 and info["comparable"]


def test_negative_and_zero_threshold_inputs():
    """thr = -1, numba: everything after box 0 is suppressed, far-apart pairs included (0 > -1).  thr = 0, cpu: the standup pre-filter
    comes first, so disjoint standups are kept, standup-overlapping pairs are dropped whether or not the polygons meet (0 >= 0)."""
    dets, _ = R.decision_pairs("car", 0.0)
    far = np.abs(dets[:, 1] - R.FAR_PAIR[1]).max(1) == 0
    assert far.sum() >= 1 and (~far).sum() > 3000
    assert (R.pair_decisions64(dets, -1.0, "numba") == 1).all()
    want = R.pair_decisions64(dets, 0.0, "cpu")
    su = R.standup_overlap64(dets[:, 0], dets[:, 1]) > 0
    inter = R.rect_inter64(dets[:, 0], dets[:, 1]) > 0
    assert np.array_equal(want == 1, su) and (su & ~inter).sum() >= 20 and (~su).sum() >= 100 and (want[far] == 2).all()
    for f in range(0, R.PAIR_FRAMES, 5):
        assert orc.rotate_nms_sorted(dets[f], -1.0, "numba").size == 1
        assert orc.rotate_nms_sorted(dets[f], 0.0, "cpu").size == want[f]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", R.REDUCE_CASES)
def test_reduce_cases_are_outside_their_bands_and_agree_with_construction_and_the_oracle(name, kind):
    case = R.reduce_case(name, kind)
    max_n = case["dets"].shape[1]
    for sem in SEMANTICS:
        info = {}
        keeps = R.reduce_reference(case, sem, info)
        assert info["ratio"] > 1.0 and info["standup"] > 1.0 and info["comparable"] and info["consulted"] > 0, info
        for f, keep in enumerate(keeps):
            built = case["built"][f]
            np.testing.assert_array_equal(keep, built[:case["post_max"]] if case["post_max"] else built)
            n = min(int(case["counts"][f]), max_n)
            np.testing.assert_array_equal(keep, _oracle_nms(kind, case["dets"][f, :n], case["thr"], sem, 1.0, case["post_max"]))
    if name == "ragged":
        assert case["counts"].tolist() == list(R.RAGGED_COUNTS) and {0, 1, 2, 63, 64, 65, 128, 129, 4095, 4096} <= set(R.RAGGED_COUNTS)
        assert case["counts"][1] == 0 and case["counts"][0] == case["counts"][2] + 1 == 4096
    if name == "chain":
        assert keeps[0].tolist() == list(range(0, 4096, 2))          # box 64 survives because box 63 is dead, at every block boundary
        dense, _ = R.greedy_nms64(case["dets"][1, :129], case["thr"], kind, "numba")
        assert dense.tolist() == list(range(0, 129, 2))              # ... and the dense loop agrees with the neighbour list
    if name == "far":
        gone = set(range(4096)) - set(keeps[0].tolist())
        assert gone == {63 * 64, 63 * 64 + 1, 63 * 64 + 17, 63 * 64 + 62, 63 * 64 + 63, 62 * 64 + 1}
    if name == "merge":
        kept = keeps[0]
        assert [int(((kept >= b * 64) & (kept < b * 64 + 64)).sum()) for b in range(8)] == [64, 1, 2, 3, 4, 5, 9, 64 - 24]
    if name == "post_block0":
        assert case["post_max"] == int((case["built"][0] < 64).sum())


@pytest.mark.parametrize("kind", KINDS)
def test_special_value_frames_have_an_oracle_answer_that_uses_every_rule(kind):
    d = R.special_frame(kind)
    assert np.isnan(d).any() and np.isinf(d).any() and (d[:, 2:4] < 0).any()
    rng = np.random.default_rng(0)
    for x in (d, d[::-1].copy()):
        for sem in SEMANTICS:
            for thr in (0.01, 0.3):
                keep = _oracle_nms(kind, x, thr, sem, 0.0)
                assert 10 < keep.size < len(d)
                assert not np.array_equal(keep, _oracle_nms(kind, np.where(np.isfinite(x), x, 1.0), thr, sem, 0.0)), "the special rows change the answer"
                if kind == "rotate":
                    # the answer does not hang on the last bit of sinf / cosf (the device's differ from the host libm's): every finite
                    # rotation moved by one ulp, at random, leaves the keep list unchanged
                    for _ in range(4):
                        moved = x.copy()
                        step = np.nextafter(x[:, 4], np.where(rng.random(len(x)) < 0.5, -np.inf, np.inf).astype(np.float32))
                        moved[:, 4] = np.where(np.isfinite(x[:, 4]), step, x[:, 4])
                        assert np.array_equal(_oracle_nms(kind, moved, thr, sem, 0.0), keep)


def test_degenerate_frame_is_exact_and_the_reference_suppresses_far_boxes_there():
    d = R.degenerate_frame()
    assert (d == np.round(d * 4) / 4).all() and (d[:, 4] == 0).all() and np.abs(d).max() <= 128                # dyadic: exact in float32
    zero = (d[:, 2] == 0) | (d[:, 3] == 0)
    assert zero.sum() == 6 and ((d[:, 2] == 0) & (d[:, 3] == 0)).sum() == 3
    iou = orc.rotate_iou(d, d, -1)
    gap = -R.standup_overlap64(d[:, None], d[None])
    assert (np.isinf(iou) & (gap > 1.0)).sum() > 50, "pairs the reference suppresses although their standup boxes are metres apart"
    for x in (d, d[::-1].copy()):
        numba, cpu = orc.rotate_nms_sorted(x, 0.3, "numba"), orc.rotate_nms_sorted(x, 0.3, "cpu")
        assert numba.size < cpu.size                   # the cpu semantics' standup pre-filter never looks at those pairs
        # with a far-apart shortcut (IoU 0 when the standup boxes are apart) the numba list would be longer
        g = -R.standup_overlap64(x[:, None], x[None])
        m = np.where(g > 1e-3, 0.0, orc.rotate_iou(x, x, -1).T)
        dead, kept = np.zeros(len(x), bool), []
        for i in range(len(x)):
            if not dead[i]:
                kept.append(i)
                with np.errstate(invalid="ignore"):
                    dead[i + 1:] |= m[i, i + 1:] > 0.3
        assert len(kept) > numba.size


# ---------------------------------------------------------------------------------------------------------------- planted mistakes
def _planted_frame(boxes, thr, kind, sem, eps, post_max, neighbours, plant):
    """A copy of greedy_nms64's loop, organised like the device (64-box blocks, 64-bit suppression words), with one mistake."""
    rot, cpu = kind == "rotate", sem == "cpu"
    n = len(boxes)
    if kind != "rotate":
        e = eps if cpu else (0.0 if plant == "eps0" else 1.0)
    neighbours = R.dense_neighbours(n) if neighbours is None else neighbours
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if dead[i] and plant != "dead":
            continue
        if not dead[i]:
            if plant == "cap_per_block":
                if post_max > 0 and len(keep) >= post_max and i % 64 == 0:
                    break
            elif post_max > 0 and len(keep) >= post_max:
                break
            keep.append(i)
        j = np.asarray(neighbours[i], int)
        j = j[j < n]
        if j.size == 0:
            continue
        if plant == "words62":
            j = j[(j >> 6) < 62]
        if rot:
            v = R.iou64(boxes[i], boxes[j])
            if cpu and plant != "no_prefilter":
                v = np.where(R.standup_overlap64(boxes[i], boxes[j]) > 0, v, -np.inf)
        else:
            v = R.aa_iou64(boxes[i], boxes[j], e)
        with np.errstate(all="ignore"):
            hit = (v >= thr) if (cpu or plant == "ge") else (v > thr)
        dead[j[hit]] = True
    return np.asarray(keep, np.int32)


def _planted(case, sem, plant):
    b, max_n, width = case["dets"].shape
    flat = case["dets"].reshape(-1, width)
    keeps = []
    for f in range(b):
        n = int(case["counts"][f])
        nb = case["neighbours"][f]
        if plant == "no_clamp":
            n, nb = min(n, len(flat) - f * max_n), None          # the rows behind max_n are the next frame's
        else:
            n = min(n, max_n)
        keeps.append(_planted_frame(flat[f * max_n:f * max_n + n], case["thr"], case["kind"], sem, 1.0, case["post_max"], nb, plant))
    return keeps


def _as_device(keeps, max_n):
    keep = np.full((len(keeps), max(max_n, max(len(k) for k in keeps))), -1, np.int32)
    for f, k in enumerate(keeps):
        keep[f, :len(k)] = k
    return keep, np.asarray([len(k) for k in keeps], np.int32)


def _fails(case, sem, plant):
    want = R.reduce_reference(case, sem)
    R.check_keep(*_as_device(_planted(case, sem, None), case["dets"].shape[1]), want)          # the unplanted copy passes
    try:
        R.check_keep(*_as_device(_planted(case, sem, plant), case["dets"].shape[1]), want)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("kind", KINDS)
def test_planted_mistakes_in_the_greedy_loop_fail_the_gpu_comparison(kind):
    assert _fails(R.reduce_case("chain", kind), "numba", "dead")                  # 3: a dead box still suppresses
    assert _fails(R.reduce_case("post1", kind), "numba", "cap_per_block")         # 4: the cap looked at once per block
    assert _fails(R.reduce_case("post65", kind), "cpu", "cap_per_block")
    assert _fails(R.reduce_case("far", kind), "numba", "words62")                 # 5: suppression words >= 62 dropped
    assert _fails(R.reduce_case("clamp", kind), "cpu", "no_clamp")                # 7: counts not clamped to max_n
    if kind == "axis_aligned":
        assert _fails(R.reduce_case("chain", kind), "numba", "eps0")              # 2: eps 0 for the +1 convention


def test_planted_comparison_and_prefilter_mistakes_fail_on_the_exact_and_two_box_inputs():
    # 1: >= for > -- every exact-threshold frame of the numba semantics
    for kind, pair, thr in (("rotate", R.EXACT_ROTATED[0.25][0], 0.25), ("rotate", R.EXACT_ROTATED[0.5][1], 0.5),
                            ("axis_aligned", R.EXACT_AA[("plus1", 0.5)], 0.5)):
        dets, cols = R.exact_pair_frames(kind, pair, 65)
        for f in range(len(cols)):
            assert _planted_frame(dets[f], thr, kind, "numba", 1.0, 0, None, None).size == 65
            assert _planted_frame(dets[f], thr, kind, "numba", 1.0, 0, None, "ge").size == 64
    # 2: eps 0 for +1 on the exact axis-aligned frames
    dets, cols = R.exact_pair_frames("axis_aligned", R.EXACT_AA[("eps0", 0.25)], 65)
    assert _planted_frame(dets[0], 0.25, "axis_aligned", "numba", 1.0, 0, None, None).size == 64          # +1: IoU 15 / 45 > 0.25
    assert _planted_frame(dets[0], 0.25, "axis_aligned", "numba", 1.0, 0, None, "eps0").size == 65        # eps 0: exactly 0.25, kept
    # 6: the standup pre-filter left out at thr = 0 (cpu): disjoint pairs are dropped too
    dets, _ = R.decision_pairs("car", 0.0)
    want = R.pair_decisions64(dets, 0.0, "cpu")
    sub = range(0, R.PAIR_FRAMES, 16)
    good = np.array([_planted_frame(dets[f], 0.0, "rotate", "cpu", 1.0, 0, None, None).size for f in sub])
    bad = np.array([_planted_frame(dets[f], 0.0, "rotate", "cpu", 1.0, 0, None, "no_prefilter").size for f in sub])
    assert np.array_equal(good, want[::16]) and not np.array_equal(bad, want[::16]) and (bad == 1).all()
