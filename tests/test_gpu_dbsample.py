"""-m gpu: the device database sampling (csrc/augment.hip sec_db_sample_*, second_amd/augment.py DeviceDatabaseSampler) against
tests/golden/dbsample.npz, recorded by EXECUTING the reference's DataBaseSamplerV2.sample_all and the merge of prep_pointcloud
(tests/golden/make_golden_dbsample.py), and against the numpy restatement of tests/dbsample_helpers.py where the reference cannot
serve (containment, the 512-box limit, hand-built frames).

Everything is compared exactly: the accepted rows are decisions on admitted inputs, the merged boxes and the surviving points are
copies, and a sampled point is one fp32 add of float32 operands, which the reference also does in float32."""
import ctypes

import numpy as np
import pytest
import torch

import augment_helpers as ah
import dbsample_helpers as dh

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
    g = np.load(dh.GOLDEN)
    return {name: dh.load_case(name, g) for name in dh.CASES}


def sampler_of(case, db, **kw):
    from second_amd.augment import DeviceDatabaseSampler, DeviceGtDatabase
    database = DeviceGtDatabase(db["boxes"], db["points"], db["offsets"], db["names"], case["class_names"])
    return DeviceDatabaseSampler(database, groups=case["groups"], rate=case["rate"], sample_importance=case["sample_importance"], **kw)


def cand_tensor(cands, k=None):
    """nested lists [F][C][..] -> int32 [F, C, K] padded with -1"""
    k = k or max([len(c) for f in cands for c in f] + [1])
    out = -np.ones((len(cands), len(cands[0]), k), np.int32)
    for f, frame in enumerate(cands):
        for c, rows in enumerate(frame):
            out[f, c, :len(rows)] = rows
    return dev(out)


def call(sampler, batch, **kw):
    return sampler(dev(batch["points"]), dev(batch["point_offsets"]), dev(batch["boxes"]), dev(batch["box_offsets"]), dev(batch["classes"]),
                   gt_mask=dev(batch["valid"]), gt_importance=dev(batch["importance"]), **kw)


def check_against(sampler, out, want, batch):
    """The sampler's outputs against a dict shaped like dbsample_helpers.chain's / the fixture's: all exact."""
    pts, po, boxes, bo, classes, mask, imp = (t.cpu().numpy() for t in out)
    last = {k: v.cpu().numpy() for k, v in sampler.last.items()}
    frames = len(bo) - 1
    ao = want["accepted_offsets"]
    np.testing.assert_array_equal(last["accepted_count"], np.diff(ao))
    for f in range(frames):
        n = ao[f + 1] - ao[f]
        np.testing.assert_array_equal(last["accepted"][f, :n], want["accepted"][ao[f]:ao[f + 1]])
        assert (last["accepted"][f, n:] == -1).all()
    np.testing.assert_array_equal(last["accepted_per_group"], want["accepted_per_group"])
    np.testing.assert_array_equal(bo, want["box_offsets"])
    g = bo[-1]
    assert boxes.shape[0] == sampler.box_rows(len(batch["boxes"]), frames) >= g
    np.testing.assert_array_equal(boxes[:g].view(np.int32), np.asarray(want["boxes"], np.float32).view(np.int32))
    np.testing.assert_array_equal(classes[:g], want["classes"])
    np.testing.assert_array_equal(mask[:g], want["mask"])
    np.testing.assert_array_equal(imp[:g].view(np.int32), np.asarray(want["importance"], np.float32).view(np.int32))
    assert (boxes[g:] == 0).all() and (classes[g:] == 0).all() and not mask[g:].any() and (imp[g:] == 0).all() and not last["sampled"][g:].any()
    np.testing.assert_array_equal(po, want["point_offsets"])
    np.testing.assert_array_equal(pts[:po[-1]].view(np.int32), np.asarray(want["points"], np.float32).view(np.int32))
    assert not sampler.overflowed()


@pytest.mark.parametrize("name", list(dh.CASES))
def test_fixture_case_exact(ops, cases, name):
    case, _, db, batch, ref = cases[name]
    sampler = sampler_of(case, db).set_candidates(cand_tensor(dh.candidates_of(ref)))
    out = call(sampler, batch)
    check_against(sampler, out, ref, batch)
    # the removal mask: the set of scene points with first_box >= 0 is the reference's points_in_rbbox(...).any(-1)
    sel = sampler.last
    first = ops.points_in_boxes(dev(batch["points"]), dev(batch["point_offsets"]), sel["boxes"], sel["box_offsets"], valid=sel["sampled"])
    removed = np.unpackbits(ref["removed"], count=len(batch["points"])).astype(bool)
    np.testing.assert_array_equal(first.cpu().numpy() >= 0, removed)
    assert torch.equal(out[0], call(sampler, batch)[0])                     # deterministic


@pytest.mark.parametrize("name", list(dh.CASES))
def test_candidates_behind_the_number_to_draw_are_ignored(cases, name):
    """Valid rows appended behind the candidates the reference drew -- wherever it got as many as it asked for, none included --
    change nothing: the device applies num_table."""
    case, _, db, batch, ref = cases[name]
    cands = dh.candidates_of(ref)
    table = dh.num_table(case["groups"], case["rate"])
    bo, grown = batch["box_offsets"], 0
    for f, frame in enumerate(cands):
        for c, (cname, _) in enumerate(case["groups"]):
            n = int((batch["classes"][bo[f]:bo[f + 1]] == case["class_names"].index(cname) + 1).sum())
            want = int(table[c][n]) if n < table.shape[1] else 0
            if len(frame[c]) == want:
                rows = [r for r, nm in enumerate(db["names"]) if nm == cname][-3:]          # (the "ab" pool has no rows that were not drawn)
                frame[c] = frame[c] + rows
                grown += len(rows)
    assert grown > 0
    sampler = sampler_of(case, db).set_candidates(cand_tensor(cands))
    check_against(sampler, call(sampler, batch), ref, batch)


def hand_case(groups, class_names, rate=1.0, importance=1.0):
    return dict(groups=groups, class_names=class_names, rate=rate, sample_importance=importance)


def hand_db(boxes, names, rs, points_each=7):
    boxes = np.array(boxes, np.float32)
    pts = [np.concatenate([rs.uniform(-0.4, 0.4, (points_each, 3)), rs.uniform(0, 1, (points_each, 1))], 1).astype(np.float32) for _ in boxes]
    return dict(boxes=boxes, points=np.concatenate(pts), offsets=np.arange(len(boxes) + 1, dtype=np.int32) * points_each, names=list(names))


def hand_batch(frames):
    """[(boxes [n, 7], classes, points [N, 4])] -> batch dict"""
    fr = [dict(points=np.asarray(p, np.float32).reshape(-1, 4), boxes=np.asarray(b, np.float32).reshape(-1, 7), classes=np.asarray(c, np.int32),
               valid=np.asarray(c, np.int32) > 0, importance=np.ones(len(c), np.float32)) for b, c, p in frames]
    return dh.concat_frames(fr)


def test_containment_counts_as_a_collision():
    """A candidate wholly inside a gt box, one wholly around a gt box, one inside a later candidate: all rejected (the compiled
    meaning of box_collision_test), as in the helper; the plain-Python reference would take them."""
    rs = np.random.RandomState(5)
    gt = [[10.0, 0, -1, 4, 4, 1.5, 0.3], [30.0, 0, -1, 1, 1, 1.5, 0.0]]
    pool = [[10.2, 0.1, -1, 1, 1, 1.5, -0.4],       # inside gt 0
            [30.1, 0.1, -1, 5, 5, 1.5, 0.2],        # around gt 1
            [50.0, 10, -1, 1, 1, 1.5, 0.1],         # inside the next candidate
            [50.2, 10.1, -1, 4, 4, 1.5, 0.5],       # around the one before: accepted, nothing later or accepted touches it
            [20.0, -20, -1, 1.7, 3.9, 1.6, 1.0]]    # free
    case, db = hand_case([("Car", 7)], ["Car"]), hand_db(pool, ["Car"] * 5, rs)
    batch = hand_batch([(gt, [1, 1], rs.uniform(60, 65, (20, 4)))])
    cands = [[[0, 1, 2, 3, 4]]]
    want = dh.chain(batch, db, case, cands)
    assert list(want["accepted"]) == [3, 4]
    assert not ah.edges_cross(ah.bev_corners(np.array(pool[:1]))[0], ah.bev_corners(np.array(gt[:1]))[0])        # containment, not crossing edges
    sampler = sampler_of(case, db).set_candidates(cand_tensor(cands))
    check_against(sampler, call(sampler, batch), want, batch)


def test_frame_over_the_box_limit_keeps_its_gt_and_accepts_nothing():
    """500 gt boxes + 13 candidates in use > 512: nothing is accepted for that frame; the frame beside it is served."""
    rs = np.random.RandomState(6)
    gx, gy = np.meshgrid(np.arange(25), np.arange(20))
    many = np.stack([100 + 3.0 * gx.reshape(-1), 3.0 * gy.reshape(-1), -np.ones(500), np.ones(500), np.ones(500), np.ones(500), np.zeros(500)], 1)
    pool = [[5.0 * i, -30, -1, 1.7, 3.9, 1.6, 0.1 * i] for i in range(15)]
    case, db = hand_case([("Car", 15)], ["Car"]), hand_db(pool, ["Car"] * 15, rs)
    batch = hand_batch([(many, [1] * 2 + [0] * 498, rs.uniform(60, 65, (30, 4))), (many[:2], [1, 1], rs.uniform(60, 65, (10, 4)))])
    cands = [[list(range(15))], [list(range(15))]]
    want = dh.chain(batch, db, case, cands)
    assert list(want["accepted_offsets"]) == [0, 0, 13] and list(want["box_offsets"]) == [0, 500, 515]
    sampler = sampler_of(case, db).set_candidates(cand_tensor(cands))
    check_against(sampler, call(sampler, batch), want, batch)


def test_three_frames_with_an_empty_one_in_the_middle():
    rs = np.random.RandomState(7)
    pool = [[5.0 + 6 * i, 3.0 * (i % 3), -1, 1.7, 3.9, 1.6, 0.2 * i] for i in range(8)]
    case, db = hand_case([("Car", 4), ("Van", 2)], ["Car", "Van"], importance=0.5), hand_db(pool, ["Car"] * 5 + ["Van"] * 3, rs)
    pts = lambda n: np.concatenate([rs.uniform(0, 50, (n, 1)), rs.uniform(-3, 9, (n, 1)), rs.uniform(-1.5, -0.5, (n, 1)), rs.uniform(0, 1, (n, 1))], 1)
    batch = hand_batch([([[5.5, 0.5, -1, 1.7, 3.9, 1.6, 0.0]], [1], pts(300)), (np.zeros((0, 7)), [], np.zeros((0, 4))),
                        ([[60.0, 0, -1, 1.7, 3.9, 1.6, 0.0], [70.0, 0, -1, 2, 5, 2, 0.0]], [2, 0], pts(290))])
    cands = [[[0, 1, 2, 3], [5, 6]], [[4, 3, 2, 1], [7, 5]], [[1, 2, 3, 4], [6, 7]]]
    want = dh.chain(batch, db, case, cands)
    assert want["removed"].any() and np.diff(want["accepted_offsets"]).min() > 0
    sampler = sampler_of(case, db).set_candidates(cand_tensor(cands))
    check_against(sampler, call(sampler, batch), want, batch)


def big_frame(rs, n=1500):
    """One frame of n points (> 4 blocks of 256) where every tenth point lies inside a pool object that will be accepted."""
    pool = [[10.0 + 8 * i, -5.0, -1, 3, 5, 2, 0.3 * i] for i in range(4)]
    db = hand_db(pool, ["Car"] * 4, rs, points_each=33)
    pts = np.concatenate([rs.uniform(0, 60, (n, 1)), rs.uniform(10, 30, (n, 1)), rs.uniform(-1.5, -0.5, (n, 1)), rs.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    for i in range(0, n, 10):
        b = np.array(pool[(i // 10) % 4])
        pts[i, :3] = b[:3] + rs.uniform(-0.3, 0.3, 3)
    return db, hand_batch([(np.zeros((0, 7)), [], pts)])


def test_removal_in_every_block_of_a_frame_of_more_than_four_blocks():
    rs = np.random.RandomState(8)
    db, batch = big_frame(rs)
    case, cands = hand_case([("Car", 4)], ["Car"]), [[[2, 0, 3, 1]]]
    want = dh.chain(batch, db, case, cands)
    removed = want["removed"]
    assert len(removed) > 4 * 256 and all(removed[i:i + 256].any() for i in range(0, len(removed), 256)) and len(want["accepted"]) == 4
    sampler = sampler_of(case, db).set_candidates(cand_tensor(cands))
    check_against(sampler, call(sampler, batch), want, batch)
    # without removal every scene point survives
    keep = sampler_of(case, db, remove_points_after_sample=False).set_candidates(cand_tensor(cands))
    check_against(keep, call(keep, batch), dh.chain(batch, db, case, cands, remove=False), batch)


def test_capacity_one_row_short_cuts_the_tail_and_raises_the_overflow_word(ops):
    rs = np.random.RandomState(9)
    db, one = big_frame(rs, 600)
    case = hand_case([("Car", 4)], ["Car"])
    batch = hand_batch([(np.zeros((0, 7)), [], one["points"]), (np.zeros((0, 7)), [], one["points"][:300])])
    cands = [[[2, 0, 3, 1]], [[1, 3, -1, -1]]]
    want = dh.chain(batch, db, case, cands)
    need = int(want["point_offsets"][-1])
    sampler = sampler_of(case, db).set_candidates(cand_tensor(cands))
    sel_args = (dev(batch["boxes"]), dev(batch["box_offsets"]), dev(batch["classes"]), sampler.database.boxes, sampler.candidates,
                sampler.class_of_group, sampler.num_table)
    sel = ops.db_sample_select(*sel_args)
    first = ops.points_in_boxes(dev(batch["points"]), dev(batch["point_offsets"]), sel["boxes"], sel["box_offsets"], valid=sel["sampled"])
    merge = lambda out, cap: ops.db_sample_merge_points(dev(batch["points"]), dev(batch["point_offsets"]), first, sampler.database.pool_points,
                                                        sampler.database.pool_offsets, sampler.database.boxes, sel["accepted"],
                                                        sel["accepted_count"], out_capacity=cap, out=out)
    sentinel = torch.full((need + 8, 4), -7.0, device="cuda")
    out, offsets, overflow = merge(sentinel.clone(), need - 1)
    assert overflow.item() == 1
    assert (out[need - 1:] == -7.0).all()                                   # nothing at or behind the capacity
    np.testing.assert_array_equal(offsets.cpu().numpy(), np.minimum(want["point_offsets"], need - 1))
    np.testing.assert_array_equal(out[:need - 1].cpu().numpy().view(np.int32), want["points"][:need - 1].view(np.int32))
    # a capacity inside the first frame: the second frame is empty, its offsets sit at the capacity
    cut = int(want["point_offsets"][1]) - 5
    out, offsets, overflow = merge(sentinel.clone(), cut)
    assert overflow.item() == 1 and (out[cut:] == -7.0).all() and list(offsets.cpu().numpy()) == [0, cut, cut]
    np.testing.assert_array_equal(out[:cut].cpu().numpy().view(np.int32), want["points"][:cut].view(np.int32))
    out, offsets, overflow = merge(sentinel.clone(), need)
    assert overflow.item() == 0 and (out[need:] == -7.0).all()
    np.testing.assert_array_equal(offsets.cpu().numpy(), want["point_offsets"])
    np.testing.assert_array_equal(out[:need].cpu().numpy().view(np.int32), want["points"].view(np.int32))
    # through the sampler
    call(sampler, batch, out_point_capacity=need - 1)
    assert sampler.overflowed()
    call(sampler, batch)
    assert not sampler.overflowed()


def identity_augmenter(sampler, num_boxes, batch_size):
    """DeviceAugmenter with no noise, no flip, no rotation, unit scale, over a range that holds every box of the fixture: whatever
    it draws, its transforms are the identity.  Its draw also draws the sampler's candidates."""
    from second_amd.augment import DeviceAugmenter
    aug = DeviceAugmenter((0, 0), (0, 0, 0), (0, 0), (1.0, 1.0), (0, 0, 0), False, False, ah.RANGE, sampler=sampler)
    aug.draw(num_boxes=sampler.box_rows(num_boxes, batch_size), batch_size=batch_size)
    assert torch.equal(aug.frame_params, dev(np.array([[0, 0, 0, 1, 0, 0, 0, 0]] * batch_size, np.float32)))
    return aug


def test_sampler_augmenter_assign_targets_chain(ops, cases):
    """sampler -> DeviceAugmenter -> ops.assign_targets: the augmenter drops the boxes whose mask is false, so with identity
    transforms its boxes are the fixture chain's masked boxes, and the targets equal the ones assigned on those."""
    case, _, db, batch, ref = cases["multi"]
    sampler = sampler_of(case, db)
    aug = identity_augmenter(sampler, len(batch["boxes"]), len(batch["box_offsets"]) - 1)
    sampler.set_candidates(cand_tensor(dh.candidates_of(ref)))
    pts, po, boxes, offs, classes = aug(dev(batch["points"]), dev(batch["point_offsets"]), dev(batch["boxes"]), dev(batch["box_offsets"]),
                                        gt_classes=dev(batch["classes"]), gt_mask=dev(batch["valid"]))
    mask = ref["mask"].astype(bool)
    kept = [int(mask[ref["box_offsets"][f]:ref["box_offsets"][f + 1]].sum()) for f in range(len(ref["box_offsets"]) - 1)]
    want_offs = np.concatenate([[0], np.cumsum(kept)]).astype(np.int32)
    np.testing.assert_array_equal(offs.cpu().numpy(), want_offs)
    g = int(want_offs[-1])
    np.testing.assert_array_equal(boxes.cpu().numpy()[:g, :6], ref["boxes"][mask][:, :6])
    np.testing.assert_array_equal(classes.cpu().numpy()[:g], ref["classes"][mask])
    np.testing.assert_array_equal(po.cpu().numpy(), ref["point_offsets"])
    np.testing.assert_array_equal(pts.cpu().numpy()[:po[-1].item()], ref["points"])
    xs, ys = np.meshgrid(np.linspace(5, 45, 6), np.linspace(-20, 20, 6))
    anchors = np.array([[x, y, -1.0, 1.6, 3.9, 1.56, r] for y, x in zip(ys.reshape(-1), xs.reshape(-1)) for r in (0.0, np.pi / 2)], np.float32)
    want_boxes = np.zeros((boxes.shape[0], 7), np.float32)
    want_boxes[:g] = boxes.cpu().numpy()[:g]
    got = ops.assign_targets(dev(anchors), boxes, offs, 0.6, 0.45)
    want = ops.assign_targets(dev(anchors), dev(want_boxes), dev(want_offs), 0.6, 0.45)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


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


def test_call_captures_into_one_chain_and_follows_new_candidates(cases):
    """DeviceAugmenter with a sampler under torch.cuda.graph on static buffers: one chain of nodes; a replay after set_candidates and
    after draw is bit-identical to the eager call with the same candidates."""
    from second_amd import runtime as rt
    case, _, db, batch, ref = cases["car"]
    frames = len(batch["box_offsets"]) - 1
    sampler = sampler_of(case, db)
    gen = torch.Generator(device="cuda")
    sampler.draw(gen.manual_seed(1), batch_size=frames)
    assert tuple(sampler.candidates.shape) == (frames, 1, 15)
    storage = sampler.candidates.data_ptr()
    aug = identity_augmenter(sampler, len(batch["boxes"]), frames)
    assert sampler.candidates.data_ptr() == storage
    args = (dev(batch["points"]), dev(batch["point_offsets"]), dev(batch["boxes"]), dev(batch["box_offsets"]))
    kw = dict(gt_classes=dev(batch["classes"]), gt_mask=dev(batch["valid"]), gt_importance=dev(batch["importance"]))
    aug(*args, **kw)                                                                # warm-up: library load, allocator, the overflow word
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with rt.capture_guard(), torch.cuda.graph(graph):
        out = aug(*args, **kw)
    nodes, edges, chain = graph_is_a_chain(graph)
    assert nodes >= 7 and edges == nodes - 1 and chain, (nodes, edges, chain)
    graph.instantiate()
    fixture = cand_tensor(dh.candidates_of(ref), k=15)
    seen = []
    for step in range(3):
        if step == 1:
            sampler.set_candidates(fixture)
        else:
            aug.draw(gen.manual_seed(2 + step))                                     # the augmenter's draw draws the sampler's candidates too
        assert sampler.candidates.data_ptr() == storage
        seen.append(sampler.candidates.clone())
        graph.replay()
        torch.cuda.synchronize()
        eager = aug(*args, **kw)
        assert all(torch.equal(a, b) for a, b in zip(out, eager)), step
        if step == 1:                                                               # the fixture's candidates: the fixture's frame counts
            kept = [int(ref["mask"][ref["box_offsets"][f]:ref["box_offsets"][f + 1]].sum()) for f in range(frames)]
            np.testing.assert_array_equal(np.diff(out[3].cpu().numpy()), kept)
            np.testing.assert_array_equal(out[1].cpu().numpy(), ref["point_offsets"])
    assert not torch.equal(seen[0], seen[2]) and not torch.equal(seen[0], seen[1])
