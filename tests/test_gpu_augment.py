"""-m gpu: the device augmentation (csrc/augment.hip, second_amd/augment.py) against tests/golden/augment.npz, recorded by EXECUTING
the reference's own functions (tests/golden/make_golden_augment.py), and against the numpy restatement of tests/augment_helpers.py
where the reference cannot serve (containment, see test_augment_host.py).

Float tolerance (from the issue): per element |err| <= 16 * 2^-24 * (|p| + |c| + |t| + 1), p the input coordinate, c the centre of the
box involved, t the sum of the translations -- about 12 fp32 roundings over the two rotations, the scale and the adds, plus the
sine / cosine error, on magnitudes bounded by those terms.  For the x and y elements the magnitude of a term is hypot(x, y) (the
rotations compute each from both), for z it is |z|: augment_helpers.point_bound.  The yaw is compared modulo 2 pi with 1e-5 rad."""
import ctypes

import numpy as np
import pytest
import torch

import augment_helpers as ah

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


@pytest.fixture(scope="module")
def cases():
    g = np.load(ah.GOLDEN)
    return {name: ah.load_case(name, g) for name in ah.CASES}


def augmenter(batch, tries):
    from second_amd.augment import DeviceAugmenter
    aug = DeviceAugmenter(ah.ROT_RANGE, ah.LOC_STD, (-0.78539816, 0.78539816), (0.95, 1.05), (0.2, 0.2, 0.2), True, True, ah.RANGE,
                          num_try=tries)
    return aug.set_noise(dev(batch["loc_noises"]), dev(batch["rot_noises"]), dev(batch["frame_params"]))


def run_chain(batch, tries, points=None):
    return augmenter(batch, tries)(dev(batch["points"]) if points is None else points, dev(batch["point_offsets"]), dev(batch["boxes"]), dev(batch["box_offsets"]),
                                   gt_classes=dev(batch["classes"]), gt_mask=dev(batch["valid"]), gt_importance=dev(batch["importance"]))


@pytest.mark.parametrize("name", list(ah.CASES))
def test_points_in_boxes_equals_reference_mask(ops, cases, name):
    batch, ref = cases[name]
    first, counts = ops.points_in_boxes(dev(batch["points"]), dev(batch["point_offsets"]), dev(batch["boxes"]), dev(batch["box_offsets"]),
                                        valid=dev(batch["valid"]), want_counts=True)
    want_first, want_counts = ah.fixture_first_and_counts(batch, ref)
    np.testing.assert_array_equal(first.cpu().numpy(), want_first)
    np.testing.assert_array_equal(counts.cpu().numpy(), want_counts)
    # without a mask every box counts: the first containing box, valid or not
    every = ops.points_in_boxes(dev(batch["points"]), dev(batch["point_offsets"]), dev(batch["boxes"]), dev(batch["box_offsets"]))
    batch_all = dict(batch, valid=np.ones_like(batch["valid"]))
    np.testing.assert_array_equal(every.cpu().numpy(), ah.fixture_first_and_counts(batch_all, ref)[0])


def test_points_in_boxes_more_boxes_than_one_lds_pass(ops):
    """300 boxes in one frame (the kernel stages 256 at a time) and a 5-float row pitch, against the helper's float64 box-frame test on
    points kept 1e-3 m off every face."""
    rs = np.random.RandomState(7)
    boxes = np.stack([rs.uniform(0, 70, 300), rs.uniform(-40, 40, 300), rs.uniform(-1.5, -0.5, 300), rs.uniform(1.5, 4, 300),
                      rs.uniform(1.5, 4, 300), rs.uniform(1.4, 2, 300), rs.uniform(-np.pi, np.pi, 300)], 1).astype(np.float32)
    pts = np.concatenate([boxes[rs.randint(0, 300, 700), :3] + rs.uniform(-1, 1, (700, 3)), rs.uniform(0, 1, (700, 2))], 1).astype(np.float32)
    pts = pts[np.abs(ah.box_frame_excess(pts, boxes)).min(1) >= 1e-3]
    mask = ah.points_in_boxes_mask(pts, boxes)
    assert (mask[:, 256:].any(1) & ~mask[:, :256].any(1)).any()          # some points are inside boxes of the second pass only
    first, counts = ops.points_in_boxes(dev(pts), dev(np.array([0, len(pts)], np.int32)), dev(boxes), dev(np.array([0, 300], np.int32)),
                                        want_counts=True)
    np.testing.assert_array_equal(first.cpu().numpy(), ah.first_set(mask, np.ones(300, bool)))
    np.testing.assert_array_equal(counts.cpu().numpy(), mask.sum(0))


@pytest.mark.parametrize("name", list(ah.CASES))
def test_noise_per_box_selects_what_the_reference_selects(ops, cases, name):
    batch, ref = cases[name]
    args = (dev(batch["boxes"]), dev(batch["box_offsets"]), dev(batch["valid"]), dev(batch["loc_noises"]), dev(batch["rot_noises"]))
    sel, loc_t, rot_t = ops.noise_per_box(*args)
    np.testing.assert_array_equal(sel.cpu().numpy(), ref["selected"])
    s = ref["selected"].astype(np.int64)
    np.testing.assert_array_equal(loc_t.cpu().numpy(), ah.select_transform(batch["loc_noises"], s, batch["valid"]))
    np.testing.assert_array_equal(rot_t.cpu().numpy(), ah.select_transform(batch["rot_noises"], s, batch["valid"]))
    again = ops.noise_per_box(*args)
    assert all(torch.equal(a, b) for a, b in zip((sel, loc_t, rot_t), again))


def test_noise_per_box_counts_containment_as_collision(ops):
    """A try wholly inside another box, and a try wholly around one: collisions (the compiled meaning of box_collision_test), as in the
    helper; the plain-Python reference would take both."""
    boxes = np.array([[10.0, 0, 0, 4, 4, 1, 0.3], [20.0, 0, 0, 1, 1, 1, 0.0], [40.0, 0, 0, 1, 1, 1, 0.2], [50.0, 0, 0, 4, 4, 1, 0.0]], np.float32)
    loc = np.zeros((4, 3, 3), np.float32)
    loc[1, 0, :2], loc[1, 1, :2] = (-9.8, 0.1), (0.5, 0.5)          # box 1: first try inside box 0, second free
    loc[3, 0, :2], loc[3, 1, :2] = (-10.1, 0.1), (-10.1, 0.2)       # box 3: two tries around box 2, the third (zero noise) free
    rot = np.zeros((4, 3), np.float32)
    valid = np.ones(4, bool)
    want = ah.noise_per_box(boxes.astype(np.float64), valid, loc.astype(np.float64), rot.astype(np.float64))
    assert list(want) == [0, 1, 0, 2]
    sel, _, _ = ops.noise_per_box(dev(boxes), dev(np.array([0, 4], np.int32)), None, dev(loc), dev(rot))
    np.testing.assert_array_equal(sel.cpu().numpy(), want)


def test_noise_per_box_frame_over_the_box_limit_is_left_alone(ops):
    """A frame with more boxes than max_boxes_per_frame gets selected = -1 and zero transforms; the frame beside it is served."""
    rs = np.random.RandomState(3)
    boxes = ah._boxes(rs, 20)
    loc, rot = rs.normal(size=(20, 4, 3)).astype(np.float32) * 0.01, np.zeros((20, 4), np.float32)
    sel, loc_t, rot_t = ops.noise_per_box(dev(boxes), dev(np.array([0, 12, 20], np.int32)), None, dev(loc), dev(rot), max_boxes_per_frame=8)
    sel = sel.cpu().numpy()
    assert (sel[:12] == -1).all() and (loc_t[:12] == 0).all() and (sel[12:] == 0).all()
    assert torch.equal(loc_t[12:], dev(loc[12:, 0]))


@pytest.mark.parametrize("name", list(ah.CASES))
def test_whole_chain_matches_reference(cases, name):
    batch, ref = cases[name]
    tries = ah.CASES[name][0]
    pts_in = dev(batch["points"])
    pts, po, boxes, offs, classes, importance = run_chain(batch, tries, points=pts_in)
    assert torch.equal(pts_in, dev(batch["points"])) and pts.data_ptr() != pts_in.data_ptr() and pts.shape == pts_in.shape and torch.equal(po, dev(batch["point_offsets"]))
    pts, boxes = pts.cpu().numpy().astype(np.float64), boxes.cpu().numpy().astype(np.float64)
    kept = np.nonzero(ref["keep"])[0]
    k = len(kept)
    # kept set, order, classes, importance, offsets, zeroed tail: exact
    np.testing.assert_array_equal(offs.cpu().numpy(), ref["offsets"])
    np.testing.assert_array_equal(classes.cpu().numpy()[:k], batch["classes"][kept])
    np.testing.assert_array_equal(importance.cpu().numpy()[:k], batch["importance"][kept])
    assert boxes.shape == batch["boxes"].shape and (boxes[k:] == 0).all()
    assert (classes.cpu().numpy()[k:] == 0).all() and (importance.cpu().numpy()[k:] == 0).all()
    # values
    np.testing.assert_array_equal(pts[:, 3], batch["points"][:, 3])                     # intensity untouched
    perr, pbound = np.abs(pts[:, :3] - ref["points"]), ah.point_bound(batch)
    berr, bbound = np.abs(boxes[:k, :6] - ref["boxes"][:, :6]), ah.box_bound(batch, kept)
    dyaw = boxes[:k, 6] - ref["boxes"][:, 6]
    dyaw = np.abs(dyaw - np.round(dyaw / (2 * np.pi)) * 2 * np.pi)
    print(f"{name}: max point err / bound {np.max(perr / pbound, initial=0):.3f}, max box err / bound {np.max(berr / bbound, initial=0):.3f}, "
          f"max yaw err {np.max(dyaw, initial=0):.2e}")
    assert (perr <= pbound).all() and (berr <= bbound).all() and (dyaw <= 1e-5).all()
    assert (np.abs(boxes[:k, 6]) <= np.pi + 1e-5).all()


def test_assign_targets_on_augmented_boxes(ops, cases):
    """ops.assign_targets on the augmenter's output and on the fixture's augmented boxes: identical labels, regression targets within
    1e-4.  Anchors: a 4 x 4 map over the range, two rotations."""
    batch, ref = cases["b5_t100"]
    _, _, boxes, offs, _ = run_chain(batch, 100)[:5]
    xs, ys = np.meshgrid(np.linspace(-52.8, 52.8, 4), np.linspace(-30, 30, 4))
    anchors = np.array([[x, y, -1.0, 1.6, 3.9, 1.56, r] for y, x in zip(ys.reshape(-1), xs.reshape(-1)) for r in (0.0, np.pi / 2)], np.float32)
    want_boxes = np.zeros_like(batch["boxes"])
    want_boxes[:len(ref["boxes"])] = ref["boxes"]
    got = ops.assign_targets(dev(anchors), boxes, offs, 0.6, 0.45)
    want = ops.assign_targets(dev(anchors), dev(want_boxes), dev(ref["offsets"]), 0.6, 0.45)
    assert torch.equal(got[0], want[0]) and (got[0] > 0).any()
    assert (got[1] - want[1]).abs().max().item() <= 1e-4


def graph_is_a_chain(graph):
    """(nodes, edges) of the captured hipGraph and whether every node has at most one successor and one predecessor."""
    hip = ctypes.CDLL("libamdhip64.so")
    g = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    e = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(e)) == 0
    src, dst = (ctypes.c_void_p * max(e.value, 1))(), (ctypes.c_void_p * max(e.value, 1))()
    assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(e)) == 0
    s, d = [src[i] for i in range(e.value)], [dst[i] for i in range(e.value)]
    return n.value, e.value, len(set(s)) == len(s) and len(set(d)) == len(d)


def test_call_captures_into_one_chain_and_follows_each_draw(cases):
    """DeviceAugmenter.__call__ under torch.cuda.graph on static buffers: two draws with different seeds, a replay after each, each
    bit-identical to the eager call with the same noise; the captured graph is one chain of kernel nodes (no side stream)."""
    from second_amd import runtime as rt
    from second_amd.augment import DeviceAugmenter
    batch, _ = cases["b5_t100"]
    args = (dev(batch["points"]), dev(batch["point_offsets"]), dev(batch["boxes"]), dev(batch["box_offsets"]))
    kw = dict(gt_classes=dev(batch["classes"]), gt_mask=dev(batch["valid"]), gt_importance=dev(batch["importance"]))
    aug = DeviceAugmenter(ah.ROT_RANGE, ah.LOC_STD, (-0.78539816, 0.78539816), (0.95, 1.05), (0.2, 0.2, 0.2), True, True, ah.RANGE, num_try=100)
    gen = torch.Generator(device="cuda")
    aug.draw(gen.manual_seed(1), num_boxes=len(batch["boxes"]), batch_size=5)
    first = [t.clone() for t in (aug.loc_noises, aug.rot_noises, aug.frame_params)]
    storage = aug.loc_noises.data_ptr()
    aug.draw(gen.manual_seed(1))
    assert all(torch.equal(a, b) for a, b in zip(first, (aug.loc_noises, aug.rot_noises, aug.frame_params)))     # same seed, same tensors
    assert aug.loc_noises.data_ptr() == storage
    std = aug.loc_noises.reshape(-1, 3).std(0).cpu().numpy()
    assert np.allclose(std, ah.LOC_STD, rtol=0.05) and ah.ROT_RANGE[0] <= aug.rot_noises.min() < aug.rot_noises.max() <= ah.ROT_RANGE[1]
    fp = aug.frame_params.cpu().numpy()
    assert set(np.unique(fp[:, :2])) <= {0.0, 1.0} and (np.abs(fp[:, 2]) <= 0.78539816).all() and ((fp[:, 3] >= 0.95) & (fp[:, 3] <= 1.05)).all()
    aug(*args, **kw)                                                                # warm-up: library load, allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with rt.capture_guard(), torch.cuda.graph(graph):
        out = aug(*args, **kw)
    nodes, edges, chain = graph_is_a_chain(graph)
    assert nodes >= 4 and edges == nodes - 1 and chain, (nodes, edges, chain)
    graph.instantiate()
    for seed in (2, 3):
        aug.draw(gen.manual_seed(seed))
        assert not torch.equal(aug.frame_params, first[2])
        graph.replay()
        torch.cuda.synchronize()
        eager = aug(*args, **kw)
        assert all(torch.equal(a, b) for a, b in zip(out, eager)), seed
        first[2] = aug.frame_params.clone()


def test_zero_noise_config_skips_the_per_object_stage(ops):
    """all.fhd / all.pp style settings: no per-object noise, no rotation, unit scale -- flips only; boxes and points flip together."""
    from second_amd.augment import DeviceAugmenter
    batch = ah.concat_frames([ah.build_frame(11, 6, 100, 1), ah.build_frame(12, 0, 10, 1)])
    aug = DeviceAugmenter((0, 0), (0, 0, 0), (0, 0), (1.0, 1.0), (0, 0, 0), True, True, ah.RANGE)
    assert aug.per_object_skipped
    aug.set_noise(frame_params=dev(np.array([[1, 1, 0, 1, 0, 0, 0, 0], [0, 1, 0, 1, 0, 0, 0, 0]], np.float32)))
    pts, _, boxes, offs, classes = aug(dev(batch["points"]), dev(batch["point_offsets"]), dev(batch["boxes"]), dev(batch["box_offsets"]))
    want = batch["points"].copy()
    want[:100, :2] *= -1
    want[100:, 1] *= -1
    np.testing.assert_array_equal(pts.cpu().numpy(), want)
    np.testing.assert_array_equal(offs.cpu().numpy(), [0, 6, 6])
    np.testing.assert_array_equal(boxes.cpu().numpy()[:, :2], -batch["boxes"][:, :2])
    assert (classes == 1).all()
    drawn = DeviceAugmenter((0, 0), (0, 0, 0), (0, 0), (1.0, 1.0), (0, 0, 0), True, False, ah.RANGE).draw(num_boxes=6, batch_size=64).frame_params
    assert (drawn[:, 1] == 0).all() and 0 < drawn[:, 0].sum() < 64 and (drawn[:, 2] == 0).all() and (drawn[:, 3] == 1).all()


def test_trainer_step_on_augmented_synthetic_input():
    """One eager DeviceTrainer.step (fp32) on augmented SYN-KITTI frames: the loss is finite; frame 1 is translated by 40 m, which
    pushes box centres over the range's far edge, and its box count falls."""
    from second_amd import synthetic as syn
    from second_amd.augment import DeviceAugmenter
    from second_amd.models import SecondDetector, CAR_FHD
    from second_amd.training import DeviceTrainer
    pts, offs = syn.batch_clouds([syn.syn_kitti_cloud(s) for s in range(2)])
    gt = np.concatenate([syn.syn_kitti_boxes(s, 12) for s in range(2)]).astype(np.float32)
    goffs = np.array([0, 12, 24], np.int32)
    aug = DeviceAugmenter((-0.78539816, 0.78539816), (1.0, 1.0, 0.5), (-0.78539816, 0.78539816), (0.95, 1.05), (0, 0, 0), False, True,
                          syn.CAR_FHD_RANGE, num_try=100)
    aug.draw(torch.Generator(device="cuda").manual_seed(0), num_boxes=24, batch_size=2)
    fp = aug.frame_params.clone()
    fp[:, 2] = 0.0
    fp[1, 4] = 40.0
    aug.set_noise(frame_params=fp)
    out = aug(dev(pts), dev(offs), dev(gt), dev(goffs))
    new_offs = out[3].cpu().numpy()
    assert (gt[12:, 0] > 45).any() and new_offs[2] - new_offs[1] < 12 and new_offs[1] <= 12, new_offs
    torch.manual_seed(0)
    tr = DeviceTrainer(SecondDetector(CAR_FHD).cuda())
    out6 = tr.step(*out)
    assert torch.isfinite(out6).all(), out6
