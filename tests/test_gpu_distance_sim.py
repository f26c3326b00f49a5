"""-m gpu: DistanceSimilarity on the device (csrc/train.hip: Sim<SEC_SIM_DISTANCE> in k_assign_max / k_assign_write,
k_region_similarity; ops.region_similarity, ops.assign_targets*(similarity=), second_amd.targets, DeviceTrainer's
``group_similarity``) against tests/golden/distance_similarity.npz (the executed reference) and the restatement of
tests/distance_sim_helpers.py (pinned to that fixture by tests/test_distance_sim_host.py).

The kernels implement the arithmetic numba compiles ("compiled" meaning of the helper).  The hand-built and lattice cases use
coordinates on a 1/8 m lattice and norms that are powers of two, where every operation of either meaning is exact: labels must
then be equal, not close."""
import numpy as np
import pytest
import torch

import distance_sim_helpers as H
import train_ref_helpers as T

pytestmark = pytest.mark.gpu

MODES = ("per_class", "all", "all_dist")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def dist(norm, rot=False, alpha=0.0):
    return dict(kind="distance", distance_norm=norm, with_rotation=rot, rotation_alpha=alpha)


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


@pytest.fixture(scope="module")
def g(golden):
    return golden("distance_similarity")


@pytest.fixture(scope="module")
def lattice():
    return T.lattice_case(1)


def _flat(frames):
    """[(gt, classes, importance)] -> device gt, offsets, classes, importance."""
    offs = np.cumsum([0] + [len(f[0]) for f in frames]).astype(np.int32)
    gt = np.concatenate([np.asarray(f[0], np.float32).reshape(-1, 7) for f in frames])
    cls = np.concatenate([np.asarray(f[1], np.int32) for f in frames])
    imp = np.concatenate([np.asarray(f[2], np.float32) for f in frames])
    return dev(gt), dev(offs), dev(cls), dev(imp)


def _compare(got, want_frames):
    labels, targets, importance = (t.cpu().numpy() for t in got)
    for f, (l, t, i) in enumerate(want_frames):
        np.testing.assert_array_equal(labels[f], l, err_msg=f"labels of frame {f}")
        np.testing.assert_array_equal(importance[f], i, err_msg=f"importance of frame {f}")
        np.testing.assert_allclose(targets[f], t, rtol=1e-5, atol=2e-6, err_msg=f"targets of frame {f}")   # test_gpu_train.py:108


def _ranges(ops, anchors, frames, begins, ids, mts, uts, sims, mask=None):
    """The device assignment and the restatement's, compared; returns the device labels."""
    gt, offs, cls, imp = _flat(frames)
    got = ops.assign_targets_per_class(dev(anchors), gt, offs, cls, list(begins), list(ids), list(mts), list(uts), gt_importance=imp,
                                       anchors_mask=None if mask is None else dev(mask), similarities=sims)
    want = [H.assign_ranges_ref(anchors, f[0], f[1], list(begins), list(ids), list(mts), list(uts), sims, f[2],
                                None if mask is None else mask[i]) for i, f in enumerate(frames)]
    _compare(got, want)
    return got[0].cpu().numpy()


def boxes(xy, r=0.0, size=(1.0, 1.0, 1.0), z=0.0):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    out = np.zeros((len(xy), 7), np.float32)
    out[:, :2], out[:, 2], out[:, 3:6], out[:, 6] = xy, z, size, r
    return out


def one_class(gt, imp=None):
    gt = np.asarray(gt, np.float32).reshape(-1, 7)
    return gt, np.ones(len(gt), np.int32), np.ones(len(gt), np.float32) if imp is None else np.asarray(imp, np.float32)


# ------------------------------------------------------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize("tag", MODES)
def test_fixture_through_assign_targets_per_class(ops, g, tag):
    """The executed reference's TargetAssigner with a DistanceSimilarity on two of three generators: per-class, assign_all (calculator 0
    = nearest IoU) and assign_all with the distance calculator first."""
    labels, targets, importance = H.fixture_expected(g, tag)
    gt, offs, cls, imp = _flat(H.fixture_frames(g))
    ids = [1, 2, 3] if tag == "per_class" else [0, 0, 0]
    sims = H.fixture_sims(g, tag)
    got = ops.assign_targets_per_class(dev(g["anchors"]), gt, offs, cls, g["class_anchor_begin"].tolist(), ids, g["matched"].tolist(),
                                       g["unmatched"].tolist(), gt_importance=imp, similarities=sims if tag == "per_class" else [sims[0]] * 3)
    _compare(got, list(zip(labels, targets, importance)))


@pytest.mark.parametrize("tag", MODES)
def test_fixture_through_device_target_assigner(g, tag):
    from second_amd import targets
    labels, tg, importance = H.fixture_expected(g, tag)
    dta = targets.DeviceTargetAssigner.from_reference(H.standin_assigner(g, tag), g["feature_map_size"].tolist())
    np.testing.assert_array_equal(dta.anchors.cpu().numpy(), g["anchors"])
    assert dta.class_anchor_begin == g["class_anchor_begin"].tolist()
    gt, offs, cls, imp = _flat(H.fixture_frames(g))
    _compare(dta.assign(gt, offs, cls, gt_importance=imp), list(zip(labels, tg, importance)))


def test_fixture_region_similarity(ops, g):
    """The [N, K] matrix: bit-equal to the compiled-meaning restatement without rotation; with rotation within rot_alpha * 2^-23 (a
    float32 sine differs from numpy's by at most one ulp of a number <= 1) plus one float32 rounding of the value."""
    begin = g["class_anchor_begin"].tolist()
    worst = 0.0
    for ci in (1, 2):
        kind, dn, rot, alpha = g[f"sim_{ci}"].tolist()
        a = g["anchors"][begin[ci]:begin[ci + 1]]
        for f in (0, 3):
            gt = g[f"gt_{f}"]
            got = ops.region_similarity(dev(a), dev(gt), "distance", distance_norm=dn, with_rotation=bool(rot), rotation_alpha=alpha).cpu().numpy()
            want = H.distance_similarity_ref(H.xyr(a), H.xyr(gt), dn, bool(rot), alpha, "compiled")
            assert got.dtype == np.float32 and got.shape == want.shape
            if not rot:
                np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
                # ... and NOT the float32 meaning, which the executed fixture holds: the kernel follows the compiled one
                assert (got != g[f"compare_{ci}_{f}"]).any()
            else:
                err = np.abs(got.astype(np.float64) - want.astype(np.float64))
                tol = alpha * 2.0 ** -23 + 0.5 * np.spacing(np.abs(want)).astype(np.float64)
                worst = max(worst, float(err.max()))
                print(f"region_similarity with rotation, class {ci} frame {f}: largest error {err.max():.3e}, tolerance there "
                      f"{tol.flat[err.argmax()]:.3e}, elements that differ {int((got != want).sum())} of {got.size}")
                assert (err <= tol).all(), float((err - tol).max())
    # nearest IoU through the same entry point: the overlaps the assignment kernels use
    a = g["anchors"][:begin[1]]
    got = ops.region_similarity(dev(a), dev(g["gt_0"])).cpu().numpy()
    want = T.iou_eps0(T.near_boxes(a), T.near_boxes(g["gt_0"]))
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    assert ops.region_similarity(dev(a), dev(np.zeros((0, 7), np.float32)), "distance", distance_norm=1.0).shape == (len(a), 0)
    with pytest.raises(ValueError):
        ops.region_similarity(dev(a), dev(g["gt_0"]), "distance", distance_norm=0.0)
    with pytest.raises(ValueError):
        ops.region_similarity(dev(a), dev(g["gt_0"]), "rotate_iou")


# ------------------------------------------------------------------------------------------------------------ 2. hand-built cases
def _matrix(ops, anchors, gt, norm):
    """Device matrix, checked bit for bit against BOTH meanings (which therefore agree)."""
    got = ops.region_similarity(dev(anchors), dev(gt), "distance", distance_norm=norm).cpu().numpy()
    for meaning in ("compiled", "float32"):
        want = H.distance_similarity_ref(H.xyr(anchors), H.xyr(gt), norm, meaning=meaning)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=meaning)
    return got


def test_negative_maximum_forces_every_tied_anchor(ops):
    """A 2 x 2 anchor range wholly inside one box's window at d / dist_norm > dist_norm: all four similarities are 1 - dist_norm =
    -0.5, the box's maximum is NEGATIVE, and create_target_np makes every anchor that ties with it positive."""
    anchors = boxes([(-1.25, -1.25), (1.25, -1.25), (-1.25, 1.25), (1.25, 1.25)])
    gt = boxes([(0, 0)])
    m = _matrix(ops, anchors, gt, 1.5)
    np.testing.assert_array_equal(m[:, 0], np.full(4, -0.5, np.float32))
    lab = _ranges(ops, anchors, [one_class(gt, [0.25])], [0, 4], [1], [0.5], [0.35], [dist(1.5)])
    np.testing.assert_array_equal(lab[0], [1, 1, 1, 1])
    # through the single-range entry point as well; forced anchors are below `matched`: importance stays 1, targets are encoded
    labels, targets, importance = ops.assign_targets(dev(anchors), dev(gt), dev(np.array([0, 1], np.int32)), 0.5, 0.35,
                                                     gt_importance=dev(np.array([0.25], np.float32)), similarity=dist(1.5))
    np.testing.assert_array_equal(labels.cpu().numpy()[0], [1, 1, 1, 1])
    np.testing.assert_array_equal(importance.cpu().numpy()[0], [1, 1, 1, 1])
    np.testing.assert_allclose(targets.cpu().numpy()[0, :, 0], np.array([1.25, -1.25, 1.25, -1.25]) / np.sqrt(2), rtol=1e-6)
    # one anchor closer than the rest: the maximum is its alone, the others are plain background
    anchors2 = np.concatenate([anchors, boxes([(1.0, 0.0)])])
    lab = _ranges(ops, anchors2, [one_class(gt)], [0, 5], [1], [0.5], [0.35], [dist(1.5)])
    np.testing.assert_array_equal(lab[0], [0, 0, 0, 0, 1])


def test_minus_one_fill_collides_with_a_genuine_minus_one(ops):
    """dist_norm = 2, dx = 2, dy = 0: the similarity is exactly -1.  A box whose maximum is 0 (some anchor outside its window, none
    with a positive similarity) gets the reference's -1 fill, and the anchors AT -1 tie with the fill: they are positive there, and
    here.  With an anchor near the box the maximum is positive and the same anchors are background."""
    anchors = boxes([(2, 0), (10, 10), (1.5, 1.5), (2, 1), (1, 1)])
    gt = boxes([(0, 0)])
    m = _matrix(ops, anchors, gt, 2.0)
    np.testing.assert_array_equal(m[:, 0], np.array([-1, 0, -1, -1, 0], np.float32))
    lab = _ranges(ops, anchors, [one_class(gt)], [0, 5], [1], [0.5], [0.35], [dist(2.0)])
    np.testing.assert_array_equal(lab[0], [1, 0, 1, 1, 0])
    near = np.concatenate([anchors, boxes([(0.5, 0)])])
    lab = _ranges(ops, near, [one_class(gt)], [0, 6], [1], [0.5], [0.35], [dist(2.0)])
    np.testing.assert_array_equal(lab[0], [0, 0, 0, 0, 0, 1])


def test_window_edge_and_clamp(ops):
    """|dx| == dist_norm is inside the window, the next float32 up is outside; min(d / dist_norm, dist_norm) clamps; unclamped
    values below zero.  dist_norm = 1.414 is no float32: the window test is made in float64 (compiled meaning), so an offset of
    float32(1.414) > 1.414 is OUTSIDE, where float32 arithmetic would put it inside."""
    up = np.nextafter(np.float32(2), np.float32(3))
    anchors = boxes([(2, 0), (up, 0), (0, -2), (0, -up), (2, 1), (1, 1), (1, 0.5), (1.5, 1), (2, 2)])
    m = _matrix(ops, anchors, boxes([(0, 0)]), 2.0)
    np.testing.assert_array_equal(m[:, 0], np.array([-1, 0, -1, 0, -1, 0, 0.375, -0.625, -1], np.float32))
    m = _matrix(ops, boxes([(3, 2), (4, 4), (4, 0), (4.5, 0)]), boxes([(0, 0)]), 4.0)
    np.testing.assert_array_equal(m[:, 0], np.array([-2.25, -3, -3, 0], np.float32))
    x = np.float32(1.414)
    assert float(x) > 1.414
    a = boxes([(x, 0), (np.nextafter(x, np.float32(0)), 0), (0, x), (0, np.nextafter(x, np.float32(0)))])
    got = ops.region_similarity(dev(a), dev(boxes([(0, 0)])), "distance", distance_norm=1.414).cpu().numpy()
    want = H.distance_similarity_ref(H.xyr(a), H.xyr(boxes([(0, 0)])), 1.414, meaning="compiled")
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0, 0] == 0 and got[2, 0] == 0 and got[1, 0] < 0 and got[3, 0] < 0


def _grid():
    """6 x 5 anchors on the integer lattice (one rotation) and boxes on the 1/8 m lattice; dist_norm = 1: every value is exact."""
    anchors = T.make_anchors(6, 5, rotations=(0.0,), size=(1.0, 1.0, 1.0))
    # [2]: no anchor in its window; [4] = [0] again; [5]: 0.75 m from its second-best anchor (similarity 0.4375: "don't care")
    gt = boxes([(0.125, 0.0), (-1.375, 1.375), (40.0, 3.0), (1.0, -1.0), (0.125, 0.0), (2.0, 0.75)])
    return anchors, gt


def test_ground_truth_without_anchor_in_its_window_and_empty_frames(ops):
    anchors, gt = _grid()
    cls = np.array([1, 1, 1, 2, 1, 1], np.int32)
    imp = np.array([0.5, 0.75, 1.25, 1.5, 2.0, 0.625], np.float32)
    frames = [(gt, cls, imp), (gt[[3]], cls[[3]], imp[[3]]), (np.zeros((0, 7), np.float32), cls[:0], imp[:0]),
              (np.zeros((0, 7), np.float32), cls[:0], imp[:0])]        # frame 1: no box of class 1; frames 2, 3: the empty batch tail
    lab = _ranges(ops, anchors, frames, [0, 30], [1], [0.5], [0.375], [dist(1.0)])
    s = H.distance_similarity_ref(H.xyr(anchors), H.xyr(gt), 1.0)
    assert (s[:, 2] == 0).all() and (s[:, [0, 1]].max(0) > 0.5).all()
    assert (lab[1:] == 0).all() and set(np.unique(lab[0]).tolist()) == {-1, 0, 1}
    # two ranges, the second one of class 2, begin no multiple of anything
    lab = _ranges(ops, anchors, frames, [0, 13, 30], [1, 2], [0.5, 0.5], [0.375, 0.375], [dist(1.0), dist(2.0)])
    assert (lab[0, 13:] == 2).any() and (lab[1, 13:] == 2).any() and (lab[1, :13] == 0).all() and not (lab[:, :13] == 2).any()


def test_masked_anchors(ops):
    """An anchors mask (prune_anchor_fn): masked anchors come back as -1 / 0 / 0 and take no part in the matching; with the anchor
    that held a box's maximum masked out, the maximum moves to the best remaining anchor, which is then the forced one."""
    anchors, gt = _grid()
    cls, imp = np.ones(6, np.int32), np.array([0.5, 0.75, 1.25, 1.5, 2.0, 0.625], np.float32)
    s = H.distance_similarity_ref(H.xyr(anchors), H.xyr(gt), 1.0)
    holder = int(s[:, 1].argmax())                                     # box 1 sits between anchors: its best, 0.72, is below `matched` = 0.75
    assert 0.375 < s[holder, 1] < 0.75
    mask = np.ones((2, 30), bool)
    mask[0, [0, 7, 29]] = False
    mask[1, [holder, 3]] = False
    frames = [(gt, cls, imp), (gt, cls, imp)]
    lab = _ranges(ops, anchors, frames, [0, 30], [1], [0.75], [0.375], [dist(1.0)], mask=mask)
    plain = _ranges(ops, anchors, frames[:1], [0, 30], [1], [0.75], [0.375], [dist(1.0)])
    assert plain[0, holder] == 1 and lab[1, holder] == -1
    runner_up = int(np.where(mask[1], s[:, 1], -np.inf).argmax())
    assert runner_up != holder and plain[0, runner_up] != 1 and lab[1, runner_up] == 1
    labels, targets, importance = ops.assign_targets(dev(anchors), *_flat(frames)[:2], 0.75, 0.375, anchors_mask=dev(mask), similarity=dist(1.0))
    np.testing.assert_array_equal(labels.cpu().numpy(), lab)
    assert (importance.cpu().numpy()[~mask] == 0).all() and (targets.cpu().numpy()[~mask] == 0).all()


# ---------------------------------------------------------------------------------------------------------- 3. layout of the launch
LAT_M, LAT_U = [0.6, 0.5, 0.5], [0.45, 0.375, 0.375]


def _lat_frames(c, pick=None, one=False):
    idx = range(len(c["gt"])) if pick is None else pick
    return [(c["gt"][i], np.ones_like(c["classes"][i]) if one else c["classes"][i], c["importance"][i]) for i in idx]


@pytest.mark.parametrize("norm", [1.0, 2.0])
def test_three_hundred_boxes_of_one_class(ops, lattice, norm):
    """874 anchors (under four workgroups, no multiple of 256) against 300, 256, 257, 0 and 1 boxes of ONE class: more than one LDS
    chunk of 256 boxes.  Coordinates on the 1/8 m lattice, the norm a power of two: every similarity is exact, many of them tie."""
    c = lattice
    frames = _lat_frames(c, one=True)
    s = H.distance_similarity_ref(H.xyr(c["anchors"]), H.xyr(c["gt"][0]), norm)
    np.testing.assert_array_equal(s, H.distance_similarity_ref(H.xyr(c["anchors"]), H.xyr(c["gt"][0]), norm, meaning="float32"))
    assert (s < 0).any() == (norm > 1) and ((s == s.max(1, keepdims=True)) & (s != 0)).sum(1).max() > 1      # argmax ties
    lab = _ranges(ops, c["anchors"], frames, [0, 874], [1], [0.5], [0.375], [dist(norm)])
    assert set(np.unique(lab[0]).tolist()) == {-1, 0, 1} and (lab[3] == 0).all()
    gt, offs, cls, imp = _flat(frames)
    labels = ops.assign_targets(dev(c["anchors"]), gt, offs, 0.5, 0.375, gt_importance=imp, similarity=dist(norm))[0]
    np.testing.assert_array_equal(labels.cpu().numpy(), lab)
    got = ops.region_similarity(dev(c["anchors"]), dev(c["gt"][0]), "distance", distance_norm=norm).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), s.view(np.uint32))


@pytest.mark.parametrize("begins", [(0, 301, 301, 874), (0, 130, 301, 874)], ids=["empty_range", "three_ranges"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "anchors_mask"])
def test_mixed_ranges_unaligned(ops, lattice, begins, masked):
    """Nearest-IoU and distance ranges in one call, begins and lengths that are no multiples of the block size, class-filtered
    ground truth (fewer than ten boxes of class 2 among 300, some past index 256), a frame without class 3, an empty frame."""
    c = lattice
    mask = None
    if masked:
        mask = np.random.default_rng(7).random((len(c["gt"]), len(c["anchors"]))) >= 0.3
    sims = [None, dist(2.0), dist(1.0)]
    lab = _ranges(ops, c["anchors"], _lat_frames(c), begins, [1, 2, 3], LAT_M, LAT_U, sims, mask=mask)
    if not masked and begins[1] != begins[2]:
        assert all((lab[0, begins[k]:begins[k + 1]] == k + 1).any() for k in range(3))
    # the ranges swapped round: distance first, nearest last
    _ranges(ops, c["anchors"], _lat_frames(c), begins, [1, 2, 3], LAT_M[::-1], LAT_U[::-1], [dist(1.0), "nearest_iou", None], mask=mask)


def test_assign_all_distance_over_ranges_and_batch_of_three(ops, lattice):
    """assign_all (class id 0) with a distance similarity: a box's maximum is taken over the anchors of ALL ranges, each range keeps
    its thresholds.  Batch 3 with an empty frame in the middle."""
    c = lattice
    frames = _lat_frames(c, pick=(1, 3, 2))
    assert len(frames[1][0]) == 0
    lab = _ranges(ops, c["anchors"], frames, (0, 130, 301, 874), [0, 0, 0], [0.5, 0.75, 0.5], [0.375, 0.5, 0.25], [dist(2.0)] * 3)
    assert (lab[1] == 0).all() and set(np.unique(lab[0]).tolist()) >= {-1, 0, 1, 2}


def test_invalid_similarities_are_refused_before_any_launch(ops, lattice, monkeypatch):
    from second_amd import runtime
    c = lattice
    gt, offs, cls, imp = _flat(_lat_frames(c, pick=(4,)))
    a = dev(c["anchors"])

    def call(ids, sims):
        return ops.assign_targets_per_class(a, gt, offs, cls, [0, 130, 301, 874], ids, LAT_M, LAT_U, similarities=sims)
    for ids, sims in (([1, 2, 3], [None, (1, 0.0, False, 0.0), None]),            # dist_norm <= 0: refused in Python already ...
                      ([0, 0, 0], [None, dist(1.0), None]),                       # assign_all uses calculator 0 for every range
                      ([0, 0, 0], [dist(1.0), dist(2.0), dist(1.0)]),
                      ([1, 1, 3], [None, dist(1.0), None])):                      # one class, two encodings of its best-similarity word
        with pytest.raises((ValueError, runtime.SecondHipError)):
            call(ids, sims)
    # ... and by the library itself: an unknown kind and a non-positive norm are SEC_E_INVALID
    l = runtime.lib()
    out = torch.empty((874, 1), device="cuda")
    assert l.sec_region_similarity_f32(runtime.ptr(a), 874, runtime.ptr(gt), 1, 2, 1.0, 0, 0.0, runtime.ptr(out), runtime.stream()) == -1
    assert l.sec_region_similarity_f32(runtime.ptr(a), 874, runtime.ptr(gt), 1, 1, 0.0, 0, 0.0, runtime.ptr(out), runtime.stream()) == -1
    assert l.sec_region_similarity_f32(runtime.ptr(a), 874, runtime.ptr(gt), 1, 1, -1.0, 0, 0.0, runtime.ptr(out), runtime.stream()) == -1
    call([1, 2, 3], [None, dist(1.0), dist(2.0)])                                 # the same arguments with valid similarities go through
    # sec_assign_targets_sim_f32 makes the same two checks itself (Python's own check switched off)
    monkeypatch.setattr(ops, "similarity_spec", lambda s: s)
    ok = (0, 0.0, False, 0.0)
    for bad in ((2, 1.0, False, 0.0), (-1, 1.0, False, 0.0), (1, 0.0, False, 0.0), (1, -2.0, False, 0.0), (1, float("nan"), False, 0.0)):
        with pytest.raises(runtime.SecondHipError, match="SEC_E_INVALID"):
            call([1, 2, 3], [ok, bad, ok])
    call([1, 2, 3], [ok, (1, 1.0, False, 0.0), ok])


# ------------------------------------------------------------------------------------------------------- 4. nothing existing moved
@pytest.mark.parametrize("ids", [[1, 2, 3], [0, 0, 0]], ids=["per_class", "all"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "anchors_mask"])
def test_nearest_iou_outputs_are_byte_identical(ops, lattice, ids, masked):
    """similarities=None takes the entry points that were there before; an all-"nearest_iou" list takes the new one and runs the
    NearestIou instantiation of the same kernels: the outputs are the same bytes."""
    c = lattice
    gt, offs, cls, imp = _flat(_lat_frames(c))
    a = dev(c["anchors"])
    mask = dev(np.random.default_rng(7).random((len(c["gt"]), len(c["anchors"]))) >= 0.3) if masked else None
    args = (a, gt, offs, cls, [0, 130, 301, 874], ids, LAT_M, LAT_U)
    base = ops.assign_targets_per_class(*args, gt_importance=imp, anchors_mask=mask)
    for sims in (None, ["nearest_iou"] * 3, [None, dict(kind="nearest_iou"), "nearest_iou"]):
        got = ops.assign_targets_per_class(*args, gt_importance=imp, anchors_mask=mask, similarities=sims)
        for x, y in zip(got, base):
            assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32))
    want = [T.assign_per_class_ref(c["anchors"], f[0], f[1], [0, 130, 301, 874], ids, LAT_M, LAT_U, gt_importance=f[2],
                                   mask=None if mask is None else mask[i].cpu().numpy()) for i, f in enumerate(_lat_frames(c))]
    _compare(base, want)
    base1 = ops.assign_targets(a, gt, offs, 0.6, 0.45, gt_classes=cls, gt_importance=imp, anchors_mask=mask)
    for sim in (None, "nearest_iou"):
        got = ops.assign_targets(a, gt, offs, 0.6, 0.45, gt_classes=cls, gt_importance=imp, anchors_mask=mask, similarity=sim)
        for x, y in zip(got, base1):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------- 5. DeviceTrainer
def _nusc_reduced(models, **extra):
    return dict(models.ALL_FHD_NUSC, point_cloud_range=[-12.8, -12.8, -5, 12.8, 12.8, 3], max_voxels=20000,
                anchor_ranges=[[-12.8, -12.8, r[2], 12.8, 12.8, r[5]] for r in models.ALL_FHD_NUSC["anchor_ranges"]],
                post_center_range=[-15, -15, -10, 15, 15, 10], block_filtering=None, **extra)


def trainer_case(anchors, begin):
    """Two frames of points and ground truth for the reduced nuScenes all.fhd config: frame 0 holds ONE pedestrian (class 6) box
    0.5 m off an anchor centre, a car and a traffic cone 0.25 m off; frame 1 a car and a bus on their anchors."""
    rng = np.random.default_rng(0)
    pts = [rng.uniform([-12.7, -12.7, -4.9, 0], [12.7, 12.7, 2.9, 1], (6000, 4)).astype(np.float32) for _ in range(2)]
    mid = lambda c: (begin[c - 1] + begin[c]) // 2 + 5               # noqa: E731  an anchor well inside the map
    ped = anchors[mid(6)].copy(); ped[0] += 0.5
    cone = anchors[mid(7) + 40].copy(); cone[1] += 0.25
    car0 = anchors[begin[0] + 300].copy(); car0[:2] += (0.1, -0.05)
    car1 = anchors[begin[0] + 420].copy(); car1[:2] += (-0.05, 0.1)
    bus = anchors[begin[2] + 200].copy()
    gts = [np.stack([car0, ped, cone]).astype(np.float32), np.stack([car1, bus]).astype(np.float32)]
    gcls = [np.array([1, 6, 7], np.int32), np.array([1, 3], np.int32)]
    return pts, gts, gcls, mid(6)


def test_device_trainer_group_similarity():
    """DeviceTrainer on the reduced ALL_FHD_NUSC of test_device_trainer_multiclass_step_runs_and_learns, stock and with
    models.NUSC_FHD_GROUP_SIMILARITY.  The pedestrian box lies 0.5 m off an anchor centre: near-box IoU with that anchor about 0.14 (far
    below 0.35: by IoU only the single best anchor of the box is forced positive), distance similarity 1 - 0.25 / 1.414 = 0.82 >= 0.5.
    Labels of both configs against the restatement; three optimisation steps; one captured step equal to the eager one."""
    from second_amd import models
    from second_amd.training import DeviceTrainer
    cfgs = {"stock": _nusc_reduced(models), "distance": _nusc_reduced(models, group_similarity=models.NUSC_FHD_GROUP_SIMILARITY)}
    labels, out6 = {}, {}
    for name, cfg in cfgs.items():
        torch.manual_seed(0)
        det = models.SecondDetector(cfg).cuda()
        tr = DeviceTrainer(det, lr=1e-3)
        assert (tr.similarities is None) == (name == "stock")
        begin, ids, mts, uts = tr.class_ranges
        anchors = det.anchors.cpu().numpy()
        pts, gts, gcls, ped_anchor = trainer_case(anchors, begin)
        args = (dev(np.concatenate(pts)), dev(np.array([0, 6000, 12000], np.int32)), dev(np.concatenate(gts)),
                dev(np.array([0, 3, 5], np.int32)), dev(np.concatenate(gcls)))
        with torch.no_grad():
            _, o6, lab = tr.forward_loss(*args)
        labels[name], out6[name] = lab.cpu().numpy(), o6.float().cpu()
        sims = cfg.get("group_similarity") or [None] * 10
        for f in range(2):
            want = H.assign_ranges_ref(anchors, gts[f], gcls[f], begin, ids, mts, uts, sims)[0]
            np.testing.assert_array_equal(labels[name][f], want, err_msg=f"{name}: labels of frame {f}")
        if name == "distance":
            losses = []
            for _ in range(3):
                tr.step(*args)
                losses.append(tr.loss_dict())
            assert all(np.isfinite(l["loss"]) for l in losses), losses
    ped = slice(begin[5], begin[6])
    s, d = labels["stock"][0, ped], labels["distance"][0, ped]
    k = ped_anchor - begin[5]
    assert s[k] == 0 and (s == 6).sum() == 1, "by near-box IoU the anchor 0.5 m off is background; only the box's best anchor is forced"
    assert d[k] == 6 and (d == 6).sum() > (s == 6).sum()
    cone = slice(begin[6], begin[7])
    assert (labels["distance"][0, cone] == 7).sum() > (labels["stock"][0, cone] == 7).sum()
    for c in (0, 1, 2, 3, 4, 7, 8, 9):                               # the nearest-IoU groups are untouched
        np.testing.assert_array_equal(labels["stock"][:, begin[c]:begin[c + 1]], labels["distance"][:, begin[c]:begin[c + 1]])
    assert not torch.allclose(out6["stock"], out6["distance"], rtol=1e-3), "other targets, other loss"
    # ---- one captured step (bf16 features, lr 0: the weights stand still) against the eager forward of a fresh trainer on the same
    # weights (the pattern and the bound of test_gpu_train_dense.py::test_captured_step_has_no_memory_of_the_previous_batch)
    torch.manual_seed(0)
    tr = DeviceTrainer(models.SecondDetector(cfgs["distance"]).cuda(), amp_dtype=torch.bfloat16, lr=0.0, weight_decay=0.0)
    replay = tr.capture_step(*args)
    captured = replay(*args).float().cpu()
    torch.cuda.synchronize()
    tr.check_overflow()
    assert torch.isfinite(captured).all()
    torch.manual_seed(0)
    tr2 = DeviceTrainer(models.SecondDetector(cfgs["distance"]).cuda(), amp_dtype=torch.bfloat16, lr=0.0, weight_decay=0.0)
    _, eager, lab = tr2.forward_loss(*args)
    np.testing.assert_array_equal(lab.cpu().numpy(), labels["distance"])
    torch.testing.assert_close(captured, eager.float().cpu(), rtol=2e-3, atol=1e-5)
