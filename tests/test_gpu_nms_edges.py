"""-m gpu: csrc/nms.hip (rotated IoU matrix, suppression masks, greedy reduce) against float64 geometry at every decision edge.

References and inputs: tests/nms_ref_helpers.py (numpy, float64; pinned to the executed reference's recorded outputs, to the fp32 oracle
and to planted mistakes by tests/test_nms_ref_host.py, which also checks on the CPU that every input used here keeps its conditions:
general position, decision bands, exact thresholds).  The inputs are generated on the CPU by name and seed and copied to the device.

Bounds (derived in the helpers' docstring; C = 4 C0 = 8.8 with C0 = 2.2 measured on the fp32 ORACLE, never on the device):
  intersection (criterion 2)   C delta P,  delta = 2^-23 (max(|x|, |y|) + max side), P = the smaller perimeter
  criteria -1, 0, 1            that interval propagated through the quotient (iou_bound)
  far-apart pairs              exactly 0;  duplicates at r = 0 on a dyadic grid: exactly 1
  keep lists, num_keep         equality -- every consulted pair of every input lies outside its band, or exactly on the threshold
Measured on an MI355X (largest |device - float64| / bound over all IoU-matrix cases; the test prints each with -s): 0.25, i.e. the
device's clipper is as far from float64 as the oracle's (C0 against C).

One defect these cases exposed is fixed in csrc/rotated_clip.hpp / nms.hip: the far-apart shortcut (standup boxes 1 mm apart => intersection
0) is wrong for a box with a side near zero, whose point-in-quad test (tolerance 1e-6 on dot products = 1e-6 / side in distance) "contains"
far-away corners: the reference suppresses a distant box there (IoU = area / 0), the numba semantics kept it
(test_zero_sided_boxes_take_the_reference_answer_at_any_distance).  Boxes with a side below 2 mm now always run the clipper (thin_box()).
"""
import numpy as np
import pytest
import torch

import nms_ref_helpers as R
from oracle import oracle as orc  # noqa: E402  (test infrastructure only: the fp32 answer for non-finite rows)

pytestmark = pytest.mark.gpu

SEMANTICS = ("numba", "cpu")
KINDS = ("rotate", "axis_aligned")


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()          # a copy: the helpers' inputs are read-only


def _nms(ops, dets, counts, thr, kind, sem, eps=1.0, post=0, exact=False):
    keep, num = ops.nms_sorted(dev(dets, np.float32), dev(counts, np.int32), thr, kind, sem, eps, post, exact_clip=exact)
    return keep.cpu().numpy(), num.cpu().numpy()


def _both(ops, dets, counts, thr, kind, sem, eps=1.0, post=0):
    """default and exact_clip: identical num_keep and kept rows; returns the default's."""
    keep, num = _nms(ops, dets, counts, thr, kind, sem, eps, post)
    keep_x, num_x = _nms(ops, dets, counts, thr, kind, sem, eps, post, exact=True)
    assert np.array_equal(num, num_x), f"default and exact_clip disagree on num_keep in frames {np.nonzero(num != num_x)[0][:8]}"
    for f in range(len(num)):
        assert np.array_equal(keep[f, :num[f]], keep_x[f, :num[f]]), f"frame {f}: default and exact_clip keep different boxes"
    return keep, num


# ---------------------------------------------------------------------------------------------------------------- a. IoU matrix
@pytest.mark.parametrize("gen,n,k", R.iou_matrix_cases(), ids=[f"{g}-{n}x{k}" for g, n, k in R.iou_matrix_cases()])
def test_rotate_iou_matrix_vs_float64(ops, gen, n, k):
    """(N, K) on both sides of the 64-column tile and of the 16-rows-per-wave split, all four criteria: every general-position pair
    within the derived bound of iou64, far-apart pairs exactly 0, the dyadic duplicate at r = 0 exactly 1."""
    b, q = R.iou_matrix_input(gen, n, k)
    for crit in (-1, 0, 1, 2):
        got = ops.rotate_iou(dev(b), dev(q), crit).cpu().numpy()
        assert got.shape == (n, k)
        ratio = R.check_iou_matrix(got, b, q, crit)
        print(f"[nms-edges] {gen} {n}x{k} criterion {crit}: |device - float64| / bound = {ratio:.3f}")
        if n * k >= 64 and crit != 2:
            assert got[-1, -1] == 1.0


# ---------------------------------------------------------------------------------------------------------------- b. equality
def _expect_exact(keep, num, n, cols, sem):
    for f, col in enumerate(cols):
        want = list(range(n)) if sem == "numba" else [i for i in range(n) if i != col]
        assert num[f] == len(want) and keep[f, :num[f]].tolist() == want, f"pair at column {col} of {n}: {sem} keeps {num[f]}"


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("thr", [0.25, 0.5])
def test_rotated_iou_equal_to_the_threshold_on_tile_edges(ops, thr, n):
    """IoU bit-equal to the threshold (dyadic pairs at r = 0, translated copies): numba (>) keeps both, cpu (>=) drops the later box,
    with the pair on the edges of the 16 x 64 mask tiles and of the reduce's 64-box blocks; the same with exact_clip."""
    for pair in R.EXACT_ROTATED[thr]:
        for shift in ((0.0, 0.0), (32.0, -64.0), (-1024.5, 512.25)):
            dets, cols = R.exact_pair_frames("rotate", pair, n, shift)
            counts = np.full(len(cols), n, np.int32)
            for sem in SEMANTICS:
                _expect_exact(*_both(ops, dets, counts, thr, "rotate", sem), n, cols, sem)


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("thr", [0.25, 0.5])
def test_axis_aligned_iou_equal_to_the_threshold_on_tile_edges(ops, thr, n):
    """Integer boxes whose +1 IoU (numba, and cpu at eps 1) or eps-0 IoU (cpu at eps 0) is exactly the threshold."""
    for conv, sem, eps in (("plus1", "numba", 1.0), ("plus1", "numba", 0.0), ("plus1", "cpu", 1.0), ("eps0", "cpu", 0.0)):
        for shift in ((0.0, 0.0), (-37.0, 512.0)):
            dets, cols = R.exact_pair_frames("axis_aligned", R.EXACT_AA[(conv, thr)], n, shift)
            _expect_exact(*_both(ops, dets, np.full(len(cols), n, np.int32), thr, "axis_aligned", sem, eps), n, cols, sem)


@pytest.mark.parametrize("kind", KINDS)
def test_items_form_takes_each_class_threshold_at_equality(ops, kind):
    """ops.nms_sorted_items with class thresholds (0.25, 0.5): each class's exact pair is decided by its own threshold."""
    n = 130
    pairs = (R.EXACT_ROTATED[0.25][0], R.EXACT_ROTATED[0.5][0]) if kind == "rotate" else (R.EXACT_AA[("plus1", 0.25)], R.EXACT_AA[("plus1", 0.5)])
    per_class = [R.exact_pair_frames(kind, p, n, (32.0, 64.0)) for p in pairs]
    dets = np.stack([pc[0] for pc in per_class], 1)                      # [7, 2, n, width]
    cols = per_class[0][1]
    counts = np.full((len(cols), 2), n, np.int32)
    thr_items = torch.tensor([0.25, 0.5], dtype=torch.float32, device="cuda")
    post = torch.zeros(2, dtype=torch.int32, device="cuda")
    for sem in SEMANTICS:
        for exact in (False, True):
            keep, num = ops.nms_sorted_items(dev(dets), dev(counts), thr_items, post, kind, sem, 1.0, exact_clip=exact)
            keep, num = keep.cpu().numpy(), num.cpu().numpy()
            for c in range(2):
                _expect_exact(keep[:, c], num[:, c], n, cols, sem)
    # swapped thresholds: class 0's pair (IoU 0.25) is below 0.5 -> kept by both semantics; class 1's (0.5) is above 0.25 -> dropped by both
    keep, num = ops.nms_sorted_items(dev(dets), dev(counts), thr_items.flip(0).contiguous(), post, kind, "numba", 1.0)
    assert (num.cpu().numpy() == np.array([n, n - 1])).all()


# ---------------------------------------------------------------------------------------------------------------- c. pair decisions
_PAIR_CASES = [(s, t) for s in R.PAIR_SHAPES for t in R.THRESHOLDS]


@pytest.mark.parametrize("shape,thr", _PAIR_CASES, ids=[f"{s}-thr{t}" for s, t in _PAIR_CASES])
def test_pair_decisions_vs_float64_and_the_screen_vs_the_clipper(ops, shape, thr):
    """4 096 two-box frames: num_keep is the pair's decision.  float64 IoU from 0 to 0.98, dense around the threshold and in
    (thr, 1.15 thr + 2e-4) where the inscribed-circle screen's margin decides; every pair outside its band (host test).
    decision == (iou64 > thr), or >= behind the standup pre-filter for cpu; default == exact_clip."""
    dets, _ = R.decision_pairs(shape, thr)
    counts = np.full(len(dets), 2, np.int32)
    for sem in SEMANTICS:
        keep, num = _both(ops, dets, counts, thr, "rotate", sem)
        want = R.pair_decisions64(dets, thr, sem)
        bad = np.nonzero(num != want)[0]
        assert bad.size == 0, (f"{bad.size} decisions differ from float64, first frame {bad[0]}: IoU "
                               f"{R.iou64(dets[bad[0], 0], dets[bad[0], 1])!r}, boxes {dets[bad[0]].tolist()}")
        assert (keep[:, 0] == 0).all() and (keep[num == 2, 1] == 1).all()


def test_negative_threshold_suppresses_everything_and_zero_threshold_keeps_disjoint_boxes(ops):
    dets, _ = R.decision_pairs("car", 0.0)
    counts = np.full(len(dets), 2, np.int32)
    _, num = _both(ops, dets, counts, -1.0, "rotate", "numba")            # 0 > -1: far-apart pairs included
    assert (num == 1).all()
    _, num = _both(ops, dets, counts, 0.0, "rotate", "cpu")               # standup pre-filter, then IoU >= 0
    assert np.array_equal(num, R.pair_decisions64(dets, 0.0, "cpu"))
    # the axis-aligned kind has no pre-filter: at thr = 0 the cpu rule (>= 0) drops everything, numba (> 0) only what overlaps
    case = R.reduce_case("post1", "axis_aligned")
    keep, num = _nms(ops, case["dets"], case["counts"], 0.0, "axis_aligned", "cpu", 1.0)
    assert (num == 1).all() and (keep[:, 0] == 0).all()
    keep, num = _nms(ops, case["dets"], case["counts"], 0.0, "axis_aligned", "numba")
    want = [R.greedy_nms64(case["dets"][f, :c], 0.0, "axis_aligned", "numba")[0] for f, c in enumerate(case["counts"])]
    R.check_keep(keep, num, want)
    keep, num = _nms(ops, case["dets"], case["counts"], -0.5, "axis_aligned", "numba")
    assert (num == 1).all()


# ---------------------------------------------------------------------------------------------------------------- d. reduce edges
_REDUCE = [(n, k) for k in KINDS for n in R.REDUCE_CASES]


@pytest.mark.parametrize("name,kind", _REDUCE, ids=[f"{n}-{k}" for n, k in _REDUCE])
def test_reduce_edges_vs_greedy_nms64(ops, name, kind):
    """Ragged batches with n in {0, 1, 2, 63, 64, 65, 128, 129, 4095, 4096}, counts > max_n, a 4 096-box chain (keep = even positions),
    kept rows of blocks 0 and 62 suppressing columns of block 63, blocks with 1, 2, 3, 4, 5 and 9 kept rows (the four-in-flight merge),
    caps at 1 / the number kept in block 0 / 64 / 65 / n + 1: num_keep exact, keep ascending and equal to greedy_nms64.
    Then the same call with row stride 8, NaN in the extra columns and NaN rows behind counts[b]: identical."""
    case = R.reduce_case(name, kind)
    dets, counts = case["dets"], case["counts"]
    b, max_n, width = dets.shape
    wide = np.full((b, max_n, 8), np.nan, np.float32)
    wide[:, :, :width] = dets
    for f in range(b):
        wide[f, min(int(counts[f]), max_n):] = np.nan
    for sem in SEMANTICS:
        want = R.reduce_reference(case, sem)
        keep, num = _both(ops, dets, counts, case["thr"], kind, sem, 1.0, case["post_max"])
        R.check_keep(keep, num, want)
        keep_w, num_w = _nms(ops, wide, counts, case["thr"], kind, sem, 1.0, case["post_max"])
        R.check_keep(keep_w, num_w, want)
    if name == "clamp":
        at_max, num_max = _nms(ops, dets, np.full(b, max_n, np.int32), case["thr"], kind, "numba", 1.0)
        R.check_keep(at_max, num_max, R.reduce_reference(case, "numba"))


# ---------------------------------------------------------------------------------------------------------------- e. workspace
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,max_n", [(65, 65), (65, 1024), (1000, 1000), (1000, 1024)])
def test_only_written_mask_words_are_read(ops, n, max_n, kind):
    """sec_nms_sorted_f32 with the test's own workspace, filled with 0xFF bytes and with zeros: the mask kernel skips the tiles below
    the diagonal and the rows >= n, so the reduce must read only what was written."""
    from second_amd import runtime as rt
    layout, nb, _ = R.reduce_layout("mixed", kind, n)
    buf = np.zeros((2, max_n, layout.shape[1]), np.float32)
    buf[0, :n] = layout
    buf[1, :n - 1] = layout[:n - 1]
    counts = np.array([n, n - 1], np.int32)
    want = [R.greedy_nms64(layout, R.SITE_THR, kind, "numba", neighbours=nb)[0],
            R.greedy_nms64(layout[:n - 1], R.SITE_THR, kind, "numba", neighbours=[x[x < n - 1] for x in nb[:n - 1]])[0]]
    l = rt.lib()
    d, c = dev(buf), dev(counts)
    nbytes = l.sec_nms_workspace_bytes(2, max_n)
    results = []
    for fill in (0xFF, 0x00):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        keep = torch.full((2, max_n), -7, dtype=torch.int32, device="cuda")
        num = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        rt.check(l.sec_nms_sorted_f32(rt.ptr(d), rt.ptr(c), 2, max_n, buf.shape[2], float(R.SITE_THR), 0 if kind == "rotate" else 1, 0,
                                      1.0, 0, rt.ptr(keep), rt.ptr(num), rt.ptr(ws), int(nbytes), rt.stream()),
                 "sec_nms_sorted_f32")
        torch.cuda.synchronize()
        results.append((keep.cpu().numpy(), num.cpu().numpy()))
        R.check_keep(*results[-1], want)
    assert np.array_equal(results[0][1], results[1][1])
    for f in range(2):
        k = results[0][1][f]
        assert np.array_equal(results[0][0][f, :k], results[1][0][f, :k]) and (results[0][0][f, k:] == -7).all()


# ---------------------------------------------------------------------------------------------------------------- f. special values
@pytest.mark.parametrize("kind", KINDS)
def test_special_values(ops, kind):
    """Rows with a NaN coordinate, NaN / negative sides, an infinite centre, side or rotation among ordinary boxes, in both orders: the
    keep list is the fp32 oracle's (comparisons with NaN are false: such a pair is never suppressed), and default == exact_clip."""
    d = R.special_frame(kind)
    buf = np.stack([d, d[::-1].copy()])
    counts = np.array([len(d), len(d)], np.int32)
    for sem in SEMANTICS:
        for thr in (0.01, 0.3):
            keep, num = _both(ops, buf, counts, thr, kind, sem, 0.0)
            want = [orc.rotate_nms_sorted(x, thr, sem) if kind == "rotate" else orc.nms_sorted(x, thr, sem, 0.0) for x in buf]
            R.check_keep(keep, num, want)


def test_zero_sided_boxes_take_the_reference_answer_at_any_distance(ops):
    """Boxes with a zero side "contain" far-away corners for the reference's point-in-quad test: it reports the far box's own area as
    the intersection (IoU = area / 0 = inf) and suppresses it, metres away.  On the dyadic r = 0 frame every operation is exact, so the
    keep lists and the IoU matrix equal the oracle's bit for bit -- no far-apart shortcut may return 0 for such a pair."""
    d = R.degenerate_frame()
    buf = np.stack([d, d[::-1].copy()])
    counts = np.array([len(d), len(d)], np.int32)
    for sem in SEMANTICS:
        for thr in (0.01, 0.3):
            keep, num = _both(ops, buf, counts, thr, "rotate", sem)
            R.check_keep(keep, num, [orc.rotate_nms_sorted(x, thr, sem) for x in buf])
    for crit in (-1, 0, 1, 2):
        got, ref = ops.rotate_iou(dev(d), dev(d), crit).cpu().numpy(), orc.rotate_iou(d, d, crit)
        assert np.array_equal(got, ref, equal_nan=True), crit
    assert np.isinf(orc.rotate_iou(d, d, -1)).sum() > 50
