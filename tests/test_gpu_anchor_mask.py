"""-m gpu: the anchor-area mask of the KITTI PointPillars configs on the device -- producing it (csrc/anchor_mask.hip), the masked
select of predict (csrc/predict.hip) and the masked target assignment (csrc/train.hip) against tests/golden/anchor_mask.npz (the
reference executed on CPU, tests/golden/make_golden_anchor_mask.py) and the restatements of tests/anchor_mask_helpers.py; then the
mask inside ``SecondDetector.forward_points``, through ``compat.accelerate_model`` and in the training step."""
import numpy as np
import pytest
import torch

import anchor_mask_helpers as H

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


@pytest.fixture(scope="module")
def ops():
    from second_amd import ops
    return ops


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN)


def _batched(coors):
    """frames of (z, y, x) -> [M, 4] int32 (b, z, y, x)"""
    return np.concatenate([np.concatenate([np.full((len(c), 1), b, np.int32), c.astype(np.int32)], 1) for b, c in enumerate(coors)]).astype(np.int32)


def _mask(ops, case, coords, num_dev, batch, t, anchors=None):
    vs, rng, grid = H.geometry(case)
    anchors = dev(H.anchors_of(case)[0]) if anchors is None else anchors
    return ops.anchor_area_mask(coords, num_dev, batch, (int(grid[1]), int(grid[0])), anchors, vs[:2], rng[:2], t)


# ------------------------------------------------------------------------------------------------------------ the mask
@pytest.mark.parametrize("name", sorted(H.CASES))
def test_mask_is_the_references_bit_for_bit(ops, golden, name):
    case = H.CASES[name]
    fx = H.load_case(golden, name)
    coords = dev(_batched(fx["coors"]))
    for t in case["thresholds"]:
        got = _mask(ops, case, coords, None, case["frames"], t)
        assert got.dtype == torch.uint8 and tuple(got.shape) == fx["masks"][t].shape
        want = fx["masks"][t].astype(np.uint8)
        g = got.cpu().numpy()
        assert np.array_equal(g, want), (name, t, int((g != want).sum()))
        assert torch.equal(got, _mask(ops, case, coords, None, case["frames"], t))          # int32 counts: the same bits every time


def test_mask_counts_only_live_in_range_rows_and_replays_from_a_graph(ops, golden):
    case = H.CASES["B"]
    fx = H.load_case(golden, "B")
    rows = _batched(fx["coors"])
    rows = rows[np.random.default_rng(0).permutation(len(rows))]                            # frames interleaved
    n = len(rows)
    want = dev(fx["masks"][1].astype(np.uint8))
    # garbage behind the count: rows of other frames' voxels that must not be counted, and wild values
    junk = np.concatenate([rows[:200], np.array([[7, 0, 3, 3], [-1, 0, 3, 3], [0, 0, 40, 3], [1, 0, 3, 72], [2, 0, -1, 5], [1, 0, 5, -2],
                                                 [2 ** 30, 0, 2 ** 30, 2 ** 30]], np.int32)])
    padded = dev(np.concatenate([rows, junk]))
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    assert torch.equal(_mask(ops, case, padded, cnt, 3, 1), want)
    # out-of-range batch index / coordinates INSIDE the count: skipped, never written through
    mixed = dev(np.concatenate([junk[200:], rows, junk[200:]]))
    assert torch.equal(_mask(ops, case, mixed, None, 3, 1), want)
    # no rows at all, and a zero count: every frame empty -> all-zero masks for any threshold >= 0
    assert not _mask(ops, case, padded, torch.zeros(1, dtype=torch.int32, device="cuda"), 3, 0).any()
    assert not _mask(ops, case, dev(np.zeros((0, 4), np.int32)), None, 3, 0).any()
    # captured once, replayed with two different counts: the count is read on the device at replay time
    anchors = dev(H.anchors_of(case)[0])
    half = n // 2
    want_half = dev(H.batch_mask_np(rows[:half], 3, H.anchors_of(case)[0], *H.geometry(case), 1))
    vs, rng, grid = H.geometry(case)
    out = torch.zeros((3, anchors.shape[0]), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.anchor_area_mask(padded, cnt, 3, (int(grid[1]), int(grid[0])), anchors, vs[:2], rng[:2], 1, out=out)       # warm-up (workspace)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.anchor_area_mask(padded, cnt, 3, (int(grid[1]), int(grid[0])), anchors, vs[:2], rng[:2], 1, out=out)
    cnt.fill_(half)
    graph.replay()
    assert torch.equal(out, want_half) and not torch.equal(want_half, want)
    cnt.fill_(n)
    graph.replay()
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------------------ the select
def _select_reference(cls, mask, k, thr):
    """stable sort by descending best logit of the KEPT anchors (ties by ascending anchor index) -> per frame (indices, scores) of
    the entries reaching the threshold, at most k.  cls [B, A, H, W, nc]."""
    b = cls.shape[0]
    nc = cls.shape[-1]
    flat = cls.float().reshape(b, -1, nc).max(-1).values
    out = []
    for f in range(b):
        kept = torch.nonzero(mask[f] != 0).flatten() if mask is not None else torch.arange(flat.shape[1], device=cls.device)
        order = kept[torch.sort(flat[f, kept], descending=True, stable=True).indices][:k]
        sc = torch.sigmoid(flat[f, order])
        n = int((sc >= thr).sum())
        out.append((order[:n], sc[:n]))
    return out


def _same_bits(a, b):
    """bit for bit, NaN included (rows behind counts hold the score of key 0, a NaN)"""
    as_int = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
    return torch.equal(as_int(a), as_int(b))


def _check_selection(got, want, tie_free):
    top_idx, top_score, top_label, counts = got
    for f, (idx, sc) in enumerate(want):
        c = int(counts[f])
        assert c == idx.numel(), (f, c, idx.numel())
        np.testing.assert_allclose(top_score[f, :c].cpu().numpy(), sc.cpu().numpy(), rtol=1e-6)
        if tie_free:
            assert torch.equal(top_idx[f, :c].long(), idx)
        else:                                       # the set and scores of rows [0, counts): ties by score may swap inside a run
            assert torch.equal(torch.sort(top_idx[f, :c].long()).values, torch.sort(idx).values)


SELECT_SHAPES = [(torch.float32, (3, 2, 32, 32, 1)),          # 32-bit keys
                 (torch.bfloat16, (3, 2, 32, 32, 3)),         # 16-bit register form, 2 048 anchors, three classes
                 (torch.float16, (3, 2, 32, 32, 3)),
                 (torch.bfloat16, (2, 2, 72, 64, 1))]         # 9 216 anchors: two chunks of 8 192 (chunked form)


def _select_inputs(dtype, shape, seed=0):
    b, a, h, w, nc = shape
    n = a * h * w
    g = torch.Generator(device="cuda").manual_seed(seed)
    thr = 0.3
    cls = torch.randn(b, n, nc, device="cuda", generator=g) * 0.5 - 4.0               # background: far below the threshold
    hot = torch.randperm(n, device="cuda", generator=g)[:400]
    mask = (torch.rand(b, n, device="cuda", generator=g) < 0.5)
    # frame 0: the masked-out anchors hold the highest logits (ignoring the mask fails), kept ones a band above the threshold
    cls[0, hot, 0] = torch.rand(400, device="cuda", generator=g) * 3.0
    mask[0, hot[:200]] = False
    cls[0, hot[:200], 0] += 5.0
    mask[0, hot[200:]] = True
    # frame 1: the mask removes every anchor above the threshold (counts == 0)
    cls[1, hot, 0] = 1.0 + torch.rand(400, device="cuda", generator=g)
    mask[1, hot] = False
    # third frame (the two-frame shape checks it through the all-ones call of the test): an all-ones mask
    if b > 2:
        cls[2, hot, nc - 1] = torch.rand(400, device="cuda", generator=g) * 4.0 - 1.0
        mask[2] = True
    return cls.to(dtype).reshape(b, a, h, w, nc).contiguous(), mask.contiguous(), thr


@pytest.mark.parametrize("dtype,shape", SELECT_SHAPES)
def test_masked_select(ops, dtype, shape):
    cls, mask, thr = _select_inputs(dtype, shape)
    b = shape[0]
    k = 1000
    want = _select_reference(cls, mask, k, thr)
    assert want[0][0].numel() >= 100 and want[1][0].numel() == 0 and (b == 2 or want[2][0].numel() >= 100)
    ignored = _select_reference(cls, None, k, thr)
    assert not torch.equal(torch.sort(ignored[0][0]).values, torch.sort(want[0][0]).values)
    for m in (mask, mask.to(torch.uint8)):                                                 # bool and uint8
        got = ops.predict_select(cls, k, thr, anchor_mask=m)
        _check_selection(got, want, tie_free=False)
        labels = cls.float().reshape(b, -1, shape[-1]).max(-1).indices
        for f in range(b):
            c = int(got[3][f])
            assert torch.equal(got[2][f, :c].long(), labels[f][got[0][f, :c].long()])
    # an all-ones mask and no mask: ops.predict_select without a mask, bit for bit (rows behind counts included)
    plain = ops.predict_select(cls, k, thr)
    ones = ops.predict_select(cls, k, thr, anchor_mask=torch.ones_like(mask))
    for p, o in zip(plain, ones):
        assert _same_bits(p, o)
    none = _masked_entry_point_without_mask(ops, cls, k, thr)
    for p, o in zip(plain, none):
        assert _same_bits(p, o)


def _masked_entry_point_without_mask(ops, cls, k, thr, lazy=None):
    """sec_predict_select_masked with a NULL mask, called directly (ops.predict_select takes this route itself for every head form but the
    cover one; tests/test_gpu_predict_edges.py drives the older sec_predict_select / sec_predict_select_lazy through ctypes)."""
    from second_amd import runtime as rt
    b, a, h, w, nc = cls.shape
    k = min(int(k), a * h * w, 1024)
    top_idx = torch.empty((b, k), dtype=torch.int32, device="cuda")
    top_score = torch.empty((b, k), dtype=torch.float32, device="cuda")
    top_label = torch.empty((b, k), dtype=torch.int32, device="cuda")
    counts = torch.empty((b,), dtype=torch.int32, device="cuda")
    keys = torch.empty((b * a * h * w,), dtype=torch.int32, device="cuda")
    live, bg = lazy if lazy is not None else (None, None)
    rc = rt.lib().sec_predict_select_masked(rt.ptr(cls), ops._strides5(cls), b, a, h, w, nc, k, float(thr), rt.ptr(keys), rt.ptr(top_idx),
                                            rt.ptr(top_score), rt.ptr(top_label), rt.ptr(counts), rt.dtype_code(cls.dtype), rt.ptr(live),
                                            rt.ptr(bg), None, rt.stream())
    rt.check(rc, "sec_predict_select_masked")
    return top_idx, top_score, top_label, counts


def test_masked_select_on_lazy_heads(ops):
    """tile_live + background: tiles that were never written read the empty frame's map; the mask applies on top."""
    dtype, shape = SELECT_SHAPES[0]
    cls, mask, thr = _select_inputs(dtype, shape, seed=3)
    b, a, h, w, nc = shape
    tiles_y, tiles_x = (h + 7) // 8, (w + 15) // 16
    g = torch.Generator(device="cuda").manual_seed(5)
    live = torch.rand(b, tiles_y * tiles_x, device="cuda", generator=g) < 0.6
    bg = (torch.randn(1, a, h, w, nc, device="cuda", generator=g) * 0.5 - 1.5).to(dtype)     # some background anchors pass the threshold
    per_pixel = live.reshape(b, tiles_y, 1, tiles_x, 1).expand(b, tiles_y, 8, tiles_x, 16).reshape(b, tiles_y * 8, tiles_x * 16)[:, :h, :w]
    materialised = torch.where(per_pixel.reshape(b, 1, h, w, 1), cls, bg.expand(b, -1, -1, -1, -1)).contiguous()
    holes = torch.where(per_pixel.reshape(b, 1, h, w, 1), cls, torch.full_like(cls, 30.0)).contiguous()    # unwritten tiles hold junk
    tile_live = (live.to(torch.int16) << 4).contiguous()
    want = _select_reference(materialised, mask, 1000, thr)
    got = ops.predict_select(holes, 1000, thr, lazy=(tile_live, bg), anchor_mask=mask)
    _check_selection(got, want, tie_free=False)
    eager = ops.predict_select(materialised, 1000, thr, anchor_mask=mask)
    for p, o in zip(eager, got):
        assert _same_bits(p, o)
    plain = ops.predict_select(holes, 1000, thr, lazy=(tile_live, bg))
    none = _masked_entry_point_without_mask(ops, holes, 1000, thr, lazy=(tile_live, bg))
    for p, o in zip(plain, none):
        assert _same_bits(p, o)


# ------------------------------------------------------------------------------------------------------------ the assignment
def _case_d(golden, name):
    case = H.CASES[name]
    n = case["frames"]
    gts = [golden[f"{name}_gt_{f}"] for f in range(n)]
    offs = np.cumsum([0] + [len(g) for g in gts]).astype(np.int32)
    cls = np.concatenate([golden[f"{name}_gt_classes_{f}"] for f in range(n)]).astype(np.int32)
    imp = np.concatenate([golden[f"{name}_gt_importance_{f}"] for f in range(n)]).astype(np.float32)
    return np.concatenate(gts).astype(np.float32), offs, cls, imp


@pytest.mark.parametrize("mode", ["per_class", "all"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_masked_assignment_matches_reference_target_assigner(ops, golden, name, mode):
    case = H.CASES[name]
    anchors = dev(H.anchors_of(case)[0])
    mask = H.load_case(golden, name)["masks"][1]
    gt, offs, cls, imp = _case_d(golden, name)
    begin = golden[f"{name}_class_anchor_begin"].tolist()
    ids = list(range(1, len(case["classes"]) + 1)) if mode == "per_class" else [0] * len(case["classes"])
    mt, ut = [c["matched"] for c in case["classes"]], [c["unmatched"] for c in case["classes"]]
    args = (anchors, dev(gt), dev(offs), dev(cls), begin, ids, mt, ut)
    labels, targets, importance = ops.assign_targets_per_class(*args, gt_importance=dev(imp), anchors_mask=dev(mask.astype(np.uint8)))
    want_l = golden[f"{name}_labels_{mode}"].astype(np.int32)
    np.testing.assert_array_equal(labels.cpu().numpy(), want_l)
    assert (want_l[~mask] == -1).all() and (want_l > 0).sum() >= 20 and (want_l[mask] == 0).any() and (want_l[mask] == -1).any()
    rows = golden[f"{name}_target_rows_{mode}"]
    want_t = np.zeros(want_l.shape + (7,), np.float32)
    want_t[rows[:, 0], rows[:, 1]] = golden[f"{name}_target_vals_{mode}"]
    np.testing.assert_allclose(targets.cpu().numpy(), want_t, rtol=1e-5, atol=2e-6)      # the tolerance of tests/test_gpu_train.py
    want_i = np.where(mask, 1.0, 0.0).astype(np.float32)
    want_i[rows[:, 0], rows[:, 1]] = golden[f"{name}_importance_pos_{mode}"]
    np.testing.assert_array_equal(importance.cpu().numpy(), want_i)
    # bool mask: the same
    again = ops.assign_targets_per_class(*args, gt_importance=dev(imp), anchors_mask=dev(mask))
    for p, o in zip((labels, targets, importance), again):
        assert torch.equal(p, o)
    # the mask matters to the anchors it keeps too (a ground truth's best overlap is taken over the kept anchors only)
    plain = ops.assign_targets_per_class(*args, gt_importance=dev(imp))
    keep = dev(mask)
    assert not torch.equal(plain[0][keep], labels[keep])
    # NULL mask == the unmasked entry point, bit for bit
    none = _masked_assign_without_mask(ops, *args, dev(imp))
    for p, o in zip(plain, none):
        assert torch.equal(p, o)
    if name == "A" and mode == "all":                  # one class: ops.assign_targets(anchors_mask=) is the same assignment
        single = ops.assign_targets(anchors, dev(gt), dev(offs), mt[0], ut[0], gt_classes=dev(cls), gt_importance=dev(imp), anchors_mask=dev(mask))
        for p, o in zip((labels, targets, importance), single):
            assert torch.equal(p, o)
        single_plain = ops.assign_targets(anchors, dev(gt), dev(offs), mt[0], ut[0], gt_classes=dev(cls), gt_importance=dev(imp))
        for p, o in zip(plain, single_plain):
            assert torch.equal(p, o)


def _masked_assign_without_mask(ops, anchors, gt, offs, cls, begin, ids, mt, ut, imp):
    import ctypes
    from second_amd import runtime as rt
    a, b, g, n = anchors.shape[0], offs.numel() - 1, gt.shape[0], len(ids)
    labels = torch.empty((b, a), dtype=torch.int32, device="cuda")
    targets = torch.empty((b, a, 7), dtype=torch.float32, device="cuda")
    importance = torch.empty((b, a), dtype=torch.float32, device="cuda")
    l = rt.lib()
    ws = rt.workspace(l.sec_assign_targets_workspace_bytes(b, a, g), anchors.device)
    rc = l.sec_assign_targets_masked_f32(rt.ptr(anchors), a, rt.ptr(gt), rt.ptr(cls), rt.ptr(imp), rt.ptr(offs), g, b, n,
                                         (ctypes.c_int * (n + 1))(*begin), (ctypes.c_int * n)(*ids), (ctypes.c_float * n)(*mt),
                                         (ctypes.c_float * n)(*ut), rt.ptr(labels), rt.ptr(targets), rt.ptr(importance), rt.ptr(ws),
                                         ws.numel(), None, rt.stream())
    rt.check(rc, "sec_assign_targets_masked_f32")
    return labels, targets, importance


# ------------------------------------------------------------------------------------------------------------ forward from points
def _cropped_cfg():
    """KITTI_PP_CAR_16 on a 128 x 128 pillar grid (64 x 64 feature map, 8 192 anchors)."""
    from second_amd.models import KITTI_PP_CAR_16
    return dict(KITTI_PP_CAR_16, name="pp_car16_cropped", point_cloud_range=[0, -10.24, -3, 20.48, 10.24, 1],
                anchor_offsets=[[0.16, -10.08, -1.78]], post_center_range=[0, -10.24, -5, 20.48, 10.24, 5], max_voxels=6000)


def _clouds(cfg, seeds, num_points, num_voxels):
    from second_amd import synthetic as syn
    return [syn.syn_kitti_cloud(s, num_points=num_points, num_voxels=num_voxels, point_cloud_range=tuple(cfg["point_cloud_range"]),
                                voxel_size=tuple(cfg["voxel_size"])) for s in seeds]


def _mask_of_coords(det, coords, batch):
    """numpy restatement on voxel coordinates [M, 4] (b, z, y, x) of a detector's own geometry"""
    vg = det.voxel_generator
    return H.batch_mask_np(coords.cpu().numpy(), batch, det.anchors.cpu().numpy(), vg.voxel_size, vg.point_cloud_range, det.grid_size,
                           det.cfg["anchor_area_threshold"])


def _as_list(out):
    return [{"box3d_lidar": out["boxes"][b][out["valid"][b]].float(), "scores": out["scores"][b][out["valid"][b]].float(),
             "label_preds": out["labels"][b][out["valid"][b]].long(), "metadata": None} for b in range(out["valid"].shape[0])]


def test_forward_points_computes_the_mask_and_predicts_with_it():
    from test_gpu_dropin_fused import _same
    from second_amd import synthetic as syn
    from second_amd.models import SecondDetector
    cfg = _cropped_cfg()
    torch.manual_seed(0)
    det = SecondDetector(cfg)
    syn.randomise_like_trained(det, seed=1)
    det = det.cuda().eval()
    det.pfn_slots = False                         # the pillar-tensor form of the PillarFeatureNet: the same features as the staged forward below
    pts, offs = syn.batch_clouds(_clouds(cfg, (0, 1), 2500, 1500))
    pts, offs = dev(pts), dev(offs)
    with torch.no_grad():
        vox = det.voxel_generator.generate_device(pts, offs)
        co = vox["coordinates"]
        one = co[:, 0] == 0
        f0 = det.voxel_feature_extractor(vox["voxels"][one], vox["num_points_per_voxel"][one], co[one])
        p0 = det.network_forward(f0, co[one], 1)
        syn.sharpen_heads(det, p0["cls_preds"].float(), p0["box_preds"].float())
        feats = det.voxel_feature_extractor(vox["voxels"], vox["num_points_per_voxel"], co)
        preds = det.network_forward(feats, co, 2)
        want_mask = _mask_of_coords(det, co, 2)
        assert want_mask.any() and not want_mask.all()          # both values occur (outside the sensor's field of view the ground is empty)
        want = H.masked_predict_torch(det, preds, det.anchors, dev(want_mask))
        unmasked = _as_list(det.predict_device(preds, 2))
        assert sum(w["scores"].shape[0] for w in want) >= 4
        for static in (False, True):
            det.last_anchors_mask = None
            got = det.forward_points(pts, offs, static=static)
            assert np.array_equal(det.last_anchors_mask.cpu().numpy(), want_mask)
            _same(_as_list(got), want, canonical=True)
        # without the mask the result is another one: anchors over empty ground score above the 0.05 threshold here
        assert any(u["scores"].shape != w["scores"].shape or not torch.allclose(u["scores"], w["scores"]) for u, w in zip(unmasked, want))
        # a config without the key behaves as before: no mask is computed
        plain = SecondDetector(dict(cfg, anchor_area_threshold=-1))
        assert plain.anchor_area_mask(co, 2) is None


# ------------------------------------------------------------------------------------------------------------ through the drop-in
@pytest.fixture(scope="module")
def pp_car16():
    """stand-in network of the full KITTI_PP_CAR_16, an example of two clouds with the numpy mask, the torch restatement's detections"""
    from reference_standin import build_voxelnet, example_of
    from second_amd import synthetic as syn
    from second_amd.models import KITTI_PP_CAR_16 as cfg
    torch.manual_seed(0)
    like = build_voxelnet(cfg)
    syn.randomise_like_trained(like, seed=1)
    like = like.eval().cuda()
    clouds = _clouds(cfg, (0, 1, 2), 9000, 6000)
    ex = example_of(like, clouds[:2], "cuda", metadata=False)
    with torch.no_grad():
        one = ex["coordinates"][:, 0] == 0
        p = like.network_forward(ex["voxels"][one], ex["num_points"][one], ex["coordinates"][one], 1)
        syn.sharpen_heads(like, p["cls_preds"].float(), p["box_preds"].float())
    state = {k: v.clone() for k, v in like.state_dict().items()}

    def make():
        net = build_voxelnet(cfg)
        net.load_state_dict(state)
        return net.eval().cuda()

    def want_of(net, example, mask):
        with torch.no_grad():
            preds = net.network_forward(example["voxels"], example["num_points"], example["coordinates"], 2)
            return H.masked_predict_torch(net, {k: v.float() for k, v in preds.items()}, net.anchors.float(), mask)
    mask = dev(_mask_of_coords(like, ex["coordinates"], 2))
    ex["anchors_mask"] = mask
    ex2 = example_of(like, clouds[1:3], "cuda", metadata=False)
    ex2["anchors_mask"] = dev(_mask_of_coords(like, ex2["coordinates"], 2))
    return make, ex, ex2, want_of


@pytest.mark.parametrize("deferred", [False, True])
def test_examples_with_anchors_mask_are_served_by_the_fused_path(pp_car16, deferred):
    from test_gpu_dropin_fused import _same
    from second_amd import compat
    make, ex, ex2, want_of = pp_car16
    net = make()
    want = want_of(net, ex, ex["anchors_mask"])
    want2 = want_of(net, ex2, ex2["anchors_mask"])
    with torch.no_grad():
        unmasked = net({k: v for k, v in ex.items() if k != "anchors_mask"})
    assert sum(w["scores"].shape[0] for w in want) >= 4
    assert ex["anchors_mask"].dtype == torch.uint8 and bool(ex["anchors_mask"].any()) and not bool(ex["anchors_mask"].all())
    compat.accelerate_model(net, deferred=deferred)
    eng = net._second_amd_engine
    assert eng.cfg["middle"] == "PointPillarsScatter" and eng.cfg["num_anchor_per_loc"] == 2
    with torch.no_grad():
        got = [dict(g) for g in net(ex)]
    assert eng.stats["captures"] == 1 and eng.stats["fused_calls"] == 1 and eng.stats["original_calls"] == 0, eng.stats
    _same(got, want, score_tol=2e-4, box_tol=5e-3, canonical=True)
    # the mask matters on this scene: anchors over empty ground pass the 0.05 score threshold when nothing drops them
    assert any(u["scores"].shape != w["scores"].shape or not torch.allclose(u["scores"], w["scores"], atol=1e-3) for u, w in zip(unmasked, want))
    lanes = eng.lanes if deferred else 1
    with torch.no_grad():
        for _ in range(lanes - 1):                # deferred: every lane captures its own session once
            [dict(g) for g in net(ex)]
        captures = eng.stats["captures"]
        assert captures == lanes
        # a bool mask: the same session, the same result
        as_bool = [dict(g) for g in net(dict(ex, anchors_mask=ex["anchors_mask"].bool()))]
        _same(as_bool, got, score_tol=0, box_tol=0)
        # another example with another mask: the graph is reused
        got2 = [dict(g) for g in net(ex2)]
    assert eng.stats["captures"] == captures and eng.stats["original_calls"] == 0, eng.stats
    _same(got2, want2, score_tol=2e-4, box_tol=5e-3, canonical=True)
    # a mask that is not [B, A] keeps the original forward
    assert not eng.accepts(dict(ex, anchors_mask=ex["anchors_mask"][:, :-1])) and not eng.accepts(dict(ex, anchors_mask=ex["anchors_mask"].float()))
    assert eng.accepts(ex) and eng.accepts({k: v for k, v in ex.items() if k != "anchors_mask"})


# ------------------------------------------------------------------------------------------------------------ training
def test_device_trainer_prunes_the_masked_out_anchors(ops):
    from second_amd import synthetic as syn
    from second_amd.models import SecondDetector
    from second_amd.training import DeviceTrainer
    cfg = _cropped_cfg()
    torch.manual_seed(0)
    det = SecondDetector(cfg).cuda()
    tr = DeviceTrainer(det, lr=1e-3)
    pts, offs = syn.batch_clouds(_clouds(cfg, (3, 4), 2500, 1500))
    pts, offs = dev(pts), dev(offs)
    rng = np.random.default_rng(0)
    anchors = det.anchors.cpu().numpy()
    coords = det.voxel_generator.generate_device(pts, offs)["coordinates"]
    mask = _mask_of_coords(det, coords, 2)
    boxes = []
    for f in range(2):                                              # ground truth on kept anchors, one box over empty ground
        b = np.concatenate([anchors[rng.choice(np.flatnonzero(mask[f]), 4, replace=False)], anchors[rng.choice(np.flatnonzero(mask[f] == 0), 1)]])
        b[:, :2] += rng.normal(0, 0.1, (5, 2)).astype(np.float32)
        boxes.append(b.astype(np.float32))
    gt, goffs = dev(np.concatenate(boxes)), dev(np.array([0, 5, 10], np.int32))
    loss, out6, labels = tr.forward_loss(pts, offs, gt, goffs)
    assert np.array_equal(det.last_anchors_mask.cpu().numpy(), mask)
    want = ops.assign_targets(det.anchors, gt, goffs, 0.6, 0.45, anchors_mask=dev(mask))[0]
    assert torch.equal(labels, want)
    assert (labels[dev(mask) == 0] == -1).all() and int((labels > 0).sum()) >= 8
    assert not torch.equal(labels, ops.assign_targets(det.anchors, gt, goffs, 0.6, 0.45)[0])
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in det.parameters())
    for p in det.parameters():
        p.grad = None
    assert np.isfinite(float(tr.step(pts, offs, gt, goffs)[0]))


def test_fused_train_step_accepts_examples_with_anchors_mask():
    """VoxelNet.loss never reads the mask (the example's labels already carry its effect): the captured training step serves such an
    example, with the loss of the same example without the entry."""
    from reference_standin import build_voxelnet, train_example_of
    from second_amd import compat, synthetic as syn
    from second_amd.models import CAR_FHD
    torch.manual_seed(0)
    net = build_voxelnet(CAR_FHD).cuda().train()
    clouds = [syn.syn_kitti_cloud(s, num_points=6000, num_voxels=5000) for s in (0, 1)]
    ex = train_example_of(net, clouds, [syn.syn_kitti_boxes(s, 10) for s in (0, 1)], torch.device("cuda"))
    compat.accelerate_model(net, train_dtype=torch.bfloat16)
    eng = net._second_amd_engine
    masked = dict(ex, anchors_mask=(ex["labels"] >= 0).to(torch.uint8))
    assert eng.accepts(masked)
    out = net(masked)
    assert eng.stats["train_calls"] == 1 and eng.stats["original_calls"] == 0, eng.stats
    assert bool(torch.isfinite(out["loss"]).all())
